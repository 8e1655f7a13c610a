"""One orientation list per particle (bioem_hip_upload_particle_orientations / bioem_hip_compare_own_orientations), on the
GPU, against the CPU oracle particle by particle: for particle p the oracle run over `p alone x p's list` IS the
reference's round 2 (one process per particle with --ReadOrientation <its list>).

Tolerances are those of tests/test_gpu_parity.py (REL_TOL, ABS_TOL or two float spacings of log P, norm / mu to 1e-4;
1e-9 relative where two groupings of one log-sum-exp are compared).  The maximising tuple must equal the oracle's for
every particle: no test here has 100 particles against the oracle, so nothing is exempted."""
import ctypes as C
import gzip
import math
import os

import numpy as np
import pytest

import oracle as orc
from test_gpu_parity import ABS_TOL, REL_TOL, assert_device_particles_match

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = math.radians(4.0)


def planted(W):
    """the orientation particle p of a synthetic workload was rendered from (synthetic.Workload.render_particles)"""
    return W.angles[(7919 * np.arange(W.nP)) % W.nOrient]


def grid_lists(W, n=1):
    from bioem_amd import refine
    return refine.compose(planted(W), refine.local_grid(n, STEP))


def random_lists(W, K, seed=5):
    """K random small rotations (up to ~8 degrees) around every particle's planted orientation, identity first"""
    from bioem_amd import refine
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(K, 3)) * 0.035
    v[0] = 0.0
    g = np.concatenate([v, np.ones((K, 1))], axis=1)
    g /= np.linalg.norm(g, axis=1)[:, None]
    return refine.compose(planted(W), g)


def plain_engine(W, nAngles, algo, write_angles=0):
    """a second handle on the workload's data: nAngles list entries at most, volu of a list of nAngles orientations"""
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import make_param_device
    pd = make_param_device(W.N, W.pd.maxDisplaceCenter, W.pd.GridSpaceCenter, nAngles, W.steps, 1, W.px)
    pd.writeAngles = int(write_angles)
    E = eng.Engine(pd, W.nP, nAngles, W.nCTF, algo=algo, device=0)
    E.upload_ctf(W.refCTF, W.ctfParam)
    E.upload_model(W.points, W.NormDen, W.px)
    E.upload_particle_maps(W.maps)
    return E, pd


def run_own(E, lists, p0=0, p1=None, raw=None, upload=True, isQuat=True):
    import bioem_amd.engine as eng
    if upload:
        E.upload_particle_orientations(lists, isQuat)
    if raw is None:
        raw = eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)[0]
    E.start_run(raw)
    E.compare_own_orientations(p0, E.nMaps if p1 is None else p1)
    E.finish_run(raw)
    pmap = raw[:E.nMaps * 40].view(eng.PROB_MAP_DTYPE)
    pang = raw[E.nMaps * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(E.nAngles, E.nMaps) if E.pd.writeAngles else None
    return raw, pmap, pang


def oracle_round2(W, E, pd, lists, sel, algo, angles=False, isQuat=True):
    """particle p of `sel` alone against lists[p] through the CPU oracle (its own particle spectra and sums, which the
    device's are asserted against on the way): [(prob entry, angle table [K] or None)], and the log P constant"""
    rsel, ssel, s2sel = assert_device_particles_match(E, W.maps, sel)
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(pd, f))
    K = lists.shape[1]
    opd.writeAngles = K if angles else 0
    pts = np.zeros(len(W.points), dtype=orc.POINT_DTYPE)
    for k in ("pos", "radius", "density"):
        pts[k] = W.points[k]
    L = orc.lib()
    out = []
    for i, p in enumerate(sel):
        want = np.zeros(1, dtype=orc.PROB_MAP_DTYPE)
        wang = np.zeros((K, 1), dtype=orc.PROB_ANGLE_DTYPE) if angles else None
        ang = np.ascontiguousarray(lists[p], dtype=np.float32)
        L.orc_init_prob(1, K, int(opd.writeAngles), want.ctypes.data, wang.ctypes.data if angles else None)
        L.orc_run(C.byref(opd), algo, pts.ctypes.data, len(pts), W.NormDen, ang.ctypes.data, K, int(isQuat), W.px, 0, 0, W.nCTF,
                  W.refCTF.ctypes.data, W.ctfParam.ctypes.data, 1, rsel[i:i + 1].ctypes.data, ssel[i:i + 1].ctypes.data,
                  s2sel[i:i + 1].ctypes.data, 0, K, want.ctypes.data, wang.ctypes.data if angles else None)
        out.append((want[0], wang[:, 0] if angles else None))
    return out, orc.logp_constant(opd)


def assert_round2_matches(got, want, const, sel):
    for p, (w, _) in zip(sel, want):
        g = got[p]
        la = np.log(g["Total"]) + g["Constoadd"] + const
        lb = np.log(w["Total"]) + w["Constoadd"] + const
        print("particle %d: log P device %.6f oracle %.6f diff %.3g" % (p, la, lb, la - lb))
        assert abs(la - lb) <= REL_TOL * abs(lb)
        assert abs(la - lb) <= max(ABS_TOL, 2.0 * float(np.spacing(np.float32(abs(lb)))))
        assert (g["orient"], g["conv"], g["cent_x"], g["cent_y"]) == (w["orient"], w["conv"], w["cent_x"], w["cent_y"])
        assert abs(g["norm"] - w["norm"]) <= 1e-4 * max(1.0, abs(w["norm"]))
        assert abs(g["mu"] - w["mu"]) <= 1e-4 * max(1.0, abs(w["mu"]))


def check_against_oracle(W, E, pd, lists, algo, sel=None, p0=0, p1=None):
    sel = list(range(W.nP)) if sel is None else sel
    want, const = oracle_round2(W, E, pd, lists, sel, algo)
    _, got, _ = run_own(E, lists, p0, p1)
    assert_round2_matches(got, want, const, sel)
    return got


# ------------------------------------------------------------------------------------------------------
# 1. oracle parity per kernel family
# ------------------------------------------------------------------------------------------------------
def _snapshot_signature(N, d, g, algo):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "selection_snapshot.txt.gz"), "rt") as f:
        for ln in f:
            a = ln.rstrip("\n").split(" ", 4)
            if (int(a[0]), int(a[1]), int(a[2]), int(a[3])) == (N, d, g, algo):
                return a[4]
    return None


FAMILY_SHAPES = [
    # N, maxD, grid, kernel, what the shape is there for
    (224, 10, 1, "k_compare_fast", "headline"),
    (128, 10, 1, "k_compare_fast", "nyquist_split"),
    (256, 10, 1, "k_compare_fast", "padded_pitch"),
    (160, 10, 1, "k_compare_fast", "split_last_block"),
    (224, 13, 1, "k_compare_fastm", "fastm"),
    (224, 20, 1, "k_compare_fastm2", "fastm2"),
    (224, 40, 1, "k_compare_wide2", "wide2_32"),
    (128, 40, 1, "k_compare_wide2", "wide2_16_nyquist"),
    (75, 10, 1, "k_compare_oddfft", "oddfft"),
    (33, 10, 2, "k_compare_rows", "rows"),
    (34, 16, 3, "k_compare_generic", "generic"),
]


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N,maxD,grid,kernel,what", FAMILY_SHAPES, ids=[s[4] for s in FAMILY_SHAPES])
def test_own_lists_against_oracle_per_family(N, maxD, grid, kernel, what, algo):
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=4, nOrient=27, nEnv=2, maxD=maxD, grid=grid, algo=algo, npts=150)
    try:
        E = W.engine  # nAngles = 27 = the length of the lists, volu of a 27-entry list
        assert E.kernel_name == kernel
        sig = _snapshot_signature(N, maxD, grid, algo)
        assert sig is not None and " x " not in sig and sig == E.kernel_signature  # the snapshot's kernel, untiled
        if what == "oddfft":
            assert sig.startswith("k_compare_oddfft<")
        check_against_oracle(W, E, W.pd, grid_lists(W), algo)
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 2. group shapes
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 2])
def test_rows_per_particle_not_a_multiple_of_four(algo):
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=7, nOrient=5, nEnv=3, algo=algo, npts=150)  # 15 rows per particle
    try:
        assert W.nCTF == 3
        check_against_oracle(W, W.engine, W.pd, random_lists(W, 5), algo)
    finally:
        W.engine.close()


@pytest.mark.parametrize("algo", [1, 2])
def test_euler_angle_lists(algo):
    """lists of Euler angles (alpha, beta, gamma, unused): the isQuat = 0 path of the projection, list entry by entry"""
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=5, nOrient=12, nEnv=2, algo=algo, npts=150)
    try:
        rng = np.random.default_rng(3)
        lists = np.zeros((W.nP, 12, 4), dtype=np.float32)
        lists[..., 0] = rng.uniform(-math.pi, math.pi, size=(W.nP, 12))
        lists[..., 1] = np.arccos(rng.uniform(-1.0, 1.0, size=(W.nP, 12)))
        lists[..., 2] = rng.uniform(-math.pi, math.pi, size=(W.nP, 12))
        sel = list(range(W.nP))
        want, const = oracle_round2(W, W.engine, W.pd, lists, sel, algo, isQuat=False)
        _, got, _ = run_own(W.engine, lists, isQuat=False)
        assert_round2_matches(got, want, const, sel)
    finally:
        W.engine.close()


def test_list_of_one_entry_and_a_single_particle():
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=9, nOrient=1, nEnv=2, npts=150)
    try:
        check_against_oracle(W, W.engine, W.pd, random_lists(W, 1), 1)
    finally:
        W.engine.close()
    W = Workload(N=64, nP=1, nOrient=27, nEnv=2, npts=150)
    try:
        check_against_oracle(W, W.engine, W.pd, grid_lists(W), 1)
    finally:
        W.engine.close()


def test_particle_range_leaves_the_other_entries_untouched():
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=10, nOrient=27, nEnv=2, npts=150, write_angles=0)
    try:
        E, pd = plain_engine(W, 27, 1, write_angles=27)
        try:
            lists = grid_lists(W)
            fresh = eng.new_prob_block(W.nP, 27, 27)[0]
            raw, got, pang = run_own(E, lists, 3, 7)
            want, const = oracle_round2(W, E, pd, lists, [3, 4, 5, 6], 1)
            assert_round2_matches(got, want, const, [3, 4, 5, 6])
            init = fresh[:W.nP * 40].view(eng.PROB_MAP_DTYPE)
            for p in (0, 1, 2, 7, 8, 9):
                assert got[p].tobytes() == init[p].tobytes()
            ainit = fresh[W.nP * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(27, W.nP)
            for p in (0, 1, 2, 7, 8, 9):
                assert pang[:, p].tobytes() == ainit[:, p].tobytes()
            assert np.all(pang[:, 3:7]["forAngles"] > 0.0)
        finally:
            E.close()
    finally:
        W.engine.close()


def test_list_that_straddles_two_batches():
    """1 500 slots in batches of 250 (the phase records say so): lists of 150 entries begin and end inside batches"""
    from bioem_amd.synthetic import Workload
    K = 150
    W = Workload(N=64, nP=10, nOrient=K, nEnv=2, npts=150)
    try:
        E = W.engine
        lists = random_lists(W, K)
        want, const = oracle_round2(W, E, W.pd, lists, list(range(W.nP)), 1)
        E.set_phase_timing(True)
        _, got, _ = run_own(E, lists)
        rec = E.phase_records()
        E.set_phase_timing(False)
        cmp_rec = rec[rec["phase"] == 2]
        assert len(cmp_rec) >= 2 and cmp_rec["iOrientBegin"][0] == 0 and cmp_rec["iOrientEnd"][-1] == W.nP * K
        assert np.array_equal(cmp_rec["iOrientBegin"][1:], cmp_rec["iOrientEnd"][:-1])
        assert any(b % K for b in cmp_rec["iOrientBegin"][1:]), "no list straddles a batch boundary"
        for ph in (0, 1):
            r = rec[rec["phase"] == ph]
            assert np.array_equal(r["iOrientBegin"], cmp_rec["iOrientBegin"])
            assert np.array_equal(r["iOrientEnd"], cmp_rec["iOrientEnd"])
        assert_round2_matches(got, want, const, list(range(W.nP)))
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 3. the same list for every particle == the all-to-all pass
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 2])
def test_same_list_for_every_particle_equals_the_all_to_all_pass(algo):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=224, nP=200, nOrient=64, nEnv=5, algo=algo)
    try:
        E = W.engine
        raw = eng.new_prob_block(W.nP, W.nOrient, 0)[0]
        E.start_run(raw)
        E.project_convolve_compare(0, W.nOrient)
        E.finish_run(raw)
        full = raw.view(eng.PROB_MAP_DTYPE)
        lists = np.ascontiguousarray(np.broadcast_to(W.angles[None], (W.nP, W.nOrient, 4)))
        raw1, own, _ = run_own(E, lists)

        def same(a, b):
            la = np.log(a["Total"]) + a["Constoadd"]
            lb = np.log(b["Total"]) + b["Constoadd"]
            print("max |dlogP| %.3g of %.3g" % (np.abs(la - lb).max(), np.abs(lb).max()))
            assert np.abs(la - lb).max() <= 1e-9 * np.abs(lb).max()
            for k in ("orient", "conv", "cent_x", "cent_y"):
                assert np.array_equal(a[k], b[k])
            assert np.array_equal(a["norm"], b["norm"]) and np.array_equal(a["mu"], b["mu"])

        same(own, full)
        raw2, _, _ = run_own(E, lists, upload=False)
        assert raw1.tobytes() == raw2.tobytes()  # no atomics, no races
        raw3 = eng.new_prob_block(W.nP, W.nOrient, 0)[0]
        E.start_run(raw3)
        E.compare_own_orientations(0, 77)
        E.compare_own_orientations(77, W.nP)
        E.finish_run(raw3)
        same(raw3.view(eng.PROB_MAP_DTYPE), own)
        # and the all-to-all entry of the same handle still gives what it gave, bit for bit
        raw4 = eng.new_prob_block(W.nP, W.nOrient, 0)[0]
        E.start_run(raw4)
        E.project_convolve_compare(0, W.nOrient)
        E.finish_run(raw4)
        assert raw4.tobytes() == raw.tobytes()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 4. angle table
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 2])
def test_angle_table_of_the_own_list_pass(algo):
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=6, nOrient=27, nEnv=3, algo=algo, npts=150)
    try:
        E, pd = plain_engine(W, 27, algo, write_angles=27)
        try:
            lists = grid_lists(W)
            sel = list(range(W.nP))
            want, const = oracle_round2(W, E, pd, lists, sel, algo, angles=True)
            _, got, pang = run_own(E, lists)
            assert_round2_matches(got, want, const, sel)
            dev = np.log(pang["forAngles"]) + pang["ConstAngle"]  # [k][p]
            for p, (_, wa) in zip(sel, want):
                ref = np.log(wa["forAngles"]) + wa["ConstAngle"]
                print("particle %d: max table diff %.3g" % (p, np.abs(dev[:, p] - ref).max()))
                assert np.abs(dev[:, p] - ref).max() <= ABS_TOL
            top = E.topk_angles(5, const)
            for p in sel:
                order = sorted(range(27), key=lambda k: (dev[k, p], k), reverse=True)[:5]
                assert list(top[p]["orient"]) == order
                assert np.array_equal(top[p]["logp"], np.log(pang["forAngles"][order, p]) + pang["ConstAngle"][order, p] + const)
        finally:
            E.close()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 5. round 1 -> round 2
# ------------------------------------------------------------------------------------------------------
def test_round_two_is_not_below_round_one():
    import bioem_amd.engine as eng
    from bioem_amd import refine
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=12, nOrient=96, nEnv=2, npts=150)
    try:
        raw = eng.new_prob_block(W.nP, W.nOrient, 0)[0]
        W.engine.start_run(raw)
        W.engine.project_convolve_compare(0, W.nOrient)
        W.engine.finish_run(raw)
        r1 = raw.view(eng.PROB_MAP_DTYPE)
        grid = refine.local_grid(1, STEP)
        G = len(grid)
        lists = refine.refine_lists(W.angles, r1, grid)
        assert np.array_equal(lists[:, 0], W.angles[r1["orient"]])  # entry 0 IS the round-1 orientation
        E, pd = plain_engine(W, G, 1)
        try:
            _, r2, _ = run_own(E, lists)
            for p in range(W.nP):
                slack = 2.0 * float(np.spacing(np.float32(abs(r1[p]["Constoadd"]))))
                print("particle %d: Constoadd round 1 %.4f round 2 %.4f" % (p, r1[p]["Constoadd"], r2[p]["Constoadd"]))
                assert r2[p]["Constoadd"] >= r1[p]["Constoadd"] - slack
            # the final log posterior of round 2 against the oracle's, formed with the oracle's own constant for the
            # handle's volume element (a list of G orientations; the CLI test holds the driver's against a run on G entries)
            want, const = oracle_round2(W, E, pd, lists, [0, 5, 11], 1)
            assert_round2_matches(r2, want, const, [0, 5, 11])
        finally:
            E.close()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------
def test_refused_configurations_leave_the_handle_usable(monkeypatch):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload

    def all_to_all_still_works(W, E):
        raw = eng.new_prob_block(W.nP, E.nAngles, 0)[0]
        E.start_run(raw)
        E.project_convolve_compare(0, W.nOrient)
        E.finish_run(raw)
        assert np.all(raw[:W.nP * 40].view(eng.PROB_MAP_DTYPE)["Total"] > 0.0)

    W = Workload(N=64, nP=3, nOrient=8, nEnv=2, npts=150)
    try:
        E = W.engine
        assert E.L.bioem_hip_compare_own_orientations(E.h, 0, 3) == 2  # no lists
        assert "no per-particle orientation lists" in E.L.bioem_hip_last_error(E.h).decode()
        big = random_lists(W, 9)
        assert E.L.bioem_hip_upload_particle_orientations(E.h, big.ctypes.data_as(C.c_void_p), 9, 1) == 2  # K > nAngles
        assert "K <= nAngles" in E.L.bioem_hip_last_error(E.h).decode()
        E.upload_particle_orientations(random_lists(W, 8), True)
        for rng in ((-1, 2), (0, 4), (2, 1)):
            assert E.L.bioem_hip_compare_own_orientations(E.h, rng[0], rng[1]) == 2
            assert "range" in E.L.bioem_hip_last_error(E.h).decode()
        all_to_all_still_works(W, E)
    finally:
        W.engine.close()
    # a shard handle
    W = Workload(N=64, nP=3, nOrient=8, nEnv=2, npts=150, blocks=2, block=0)
    try:
        E = W.engine
        lst = random_lists(W, 8)
        assert E.L.bioem_hip_upload_particle_orientations(E.h, lst.ctypes.data_as(C.c_void_p), 8, 1) == 2
        assert "shard" in E.L.bioem_hip_last_error(E.h).decode()
        all_to_all_still_works(W, E)
    finally:
        W.engine.close()
    # a tiled wide window
    sig = C.create_string_buffer(256)
    assert eng.load_library().bioem_hip_plan(128, 60, 1, 1, sig, 256) == 0 and b" tiles of " in sig.value
    W = Workload(N=128, nP=2, nOrient=4, nEnv=1, maxD=60, npts=150)
    try:
        E = W.engine
        lst = random_lists(W, 4)
        assert E.L.bioem_hip_upload_particle_orientations(E.h, lst.ctypes.data_as(C.c_void_p), 4, 1) == 2
        assert "tiled" in E.L.bioem_hip_last_error(E.h).decode()
        all_to_all_still_works(W, E)
    finally:
        W.engine.close()
    # BIOEM_CC_DIRECT=1
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    W = Workload(N=64, nP=3, nOrient=8, nEnv=2, npts=150)
    try:
        E = W.engine
        assert E.kernel_name == "k_compare_direct"
        lst = random_lists(W, 8)
        assert E.L.bioem_hip_upload_particle_orientations(E.h, lst.ctypes.data_as(C.c_void_p), 8, 1) == 2
        assert "BIOEM_CC_DIRECT" in E.L.bioem_hip_last_error(E.h).decode()
        all_to_all_still_works(W, E)
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 7. command line: --RefineOrientations
# ------------------------------------------------------------------------------------------------------
def _write_quaternions(path, q):
    with open(path, "w") as f:
        f.write("%d\n" % len(q))
        for r in q:
            f.write("".join("%11.8f " % float(v) for v in r) + "\n")  # four 12-character columns
    return np.array([[np.float32(float("%11.8f" % float(v))) for v in r] for r in q], dtype=np.float32)  # as read back


@pytest.mark.parametrize("name,algo", [("g2_n128", 2), ("g10_n64", 1)])
def test_cli_refine_orientations(name, algo, tmp_path):
    """OutputFile is what a run without the option writes, byte for byte; every particle of OutputFile_Round2 is what
    this CLI prints for that particle alone with its list (best of round 1 (x) grid, written here with refine.compose)
    through --ReadOrientation."""
    import subprocess

    import io_formats as iof
    from bioem_amd import refine
    from golden_util import load_case, write_case_inputs
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"
    case = load_case(name)
    d = tmp_path
    base = [exe, "--Inputfile", os.path.join(case["dir"], "param.txt")]
    inputs = write_case_inputs(case, d)
    env = dict(os.environ, BIOEM_ALGO=str(algo), BIOEM_GPUS="1")
    env.update(case["env"])

    def run(args):
        r = subprocess.run(base + args, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]

    grid = _write_quaternions(d / "grid.txt", refine.local_grid(1, STEP))
    run(inputs + ["--OutputFile", "plain.txt"])
    run(inputs + ["--OutputFile", "out.txt", "--RefineOrientations", "grid.txt"])
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    r1 = iof.parse_output_probabilities(open(d / "out.txt").read())
    r2 = iof.parse_output_probabilities(open(d / "out.txt_Round2").read())
    angles = np.array([[np.float32(float(ln[12 * c:12 * c + 12])) for c in range(4)] for ln in case["orient_lines"]],
                      dtype=np.float32)
    nP = len(case["maps"])
    assert len(r1) == nP and len(r2) == nP
    margs = inputs[:inputs.index("--Particlesfile")]
    for p in range(nP):
        # the round-1 orientation of particle p: the list entry the printed (4 decimals) quaternion names
        dist = np.abs(angles - np.array(r1[p]["angles"], dtype=np.float64)).max(axis=1)
        best = int(np.argmin(dist))
        assert dist[best] <= 5.1e-5 and np.sum(dist <= 5.1e-5) == 1
        lst = refine.compose(angles[best:best + 1], grid)[0]
        _write_quaternions(d / ("list%d.txt" % p), lst)
        iof.write_text_particles(os.path.join(str(d), "one%d.txt" % p), case["maps"][p:p + 1])
        run(margs + ["--Particlesfile", "one%d.txt" % p, "--ReadOrientation", "list%d.txt" % p, "--OutputFile",
                     "single%d.txt" % p])
        s = iof.parse_output_probabilities(open(d / ("single%d.txt" % p)).read())[0]
        m = r2[p]
        print("particle %d: round 1 %.4f round 2 %.4f alone %.4f" % (p, r1[p]["logp"], m["logp"], s["logp"]))
        assert abs(m["logp"] - s["logp"]) <= REL_TOL * abs(s["logp"])
        assert abs(m["logp"] - s["logp"]) <= max(ABS_TOL, 2.0 * float(np.spacing(np.float32(abs(s["logp"])))))
        assert (m["angles"], m["ctf"], m["cx"], m["cy"]) == (s["angles"], s["ctf"], s["cx"], s["cy"])
        assert abs(m["norm"] - s["norm"]) <= 1e-4 * max(1.0, abs(s["norm"]))
        assert abs(m["mu"] - s["mu"]) <= 1e-4 * max(1.0, abs(s["mu"]))
