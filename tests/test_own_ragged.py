"""Own orientation lists of any length (bioem_hip_upload_particle_orientation_lists) and their comparison in one launch
per batch (k_compare_fast_own), on the GPU against the CPU oracle particle by particle: for particle p the oracle run
over `p alone x p's list` IS the reference's round 2 (one process per particle with --ReadOrientation <its list>).

Workloads and helpers as in tests/test_own_lists.py.  Tolerances are those of tests/test_gpu_parity.py (REL_TOL, ABS_TOL
or two float spacings of log P, norm / mu to 1e-4); the maximising tuple must equal the oracle's for every particle
tested, nothing is exempted.  Where two launch modes or two uploads are compared the probability blocks are equal byte
for byte: a wave computes one (particle, row) pair by the same instructions whichever launch it belongs to."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import oracle as orc
from test_gpu_parity import ABS_TOL, assert_device_particles_match
from test_own_lists import assert_round2_matches, plain_engine, random_lists, run_own

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 7, 0, 27, 2, 5)


def ragged_lists(W, lengths, seed=5):
    """lists[p] = the first lengths[p] of random small rotations around particle p's planted orientation, identity first"""
    full = random_lists(W, max(1, max(lengths)), seed)
    return [np.ascontiguousarray(full[p, :n]) for p, n in enumerate(lengths)]


def run_ragged(E, lists, p0=0, p1=None, raw=None, upload=True, launch="batch"):
    """upload (with the handle asked for one comparison launch per batch, which is opt-in -- or for `launch`) and run;
    upload=False: the pass once more, on the lists and in the mode the handle has"""
    import bioem_amd.engine as eng
    if upload:
        E.set_own_launch(launch)
        E.upload_particle_orientation_lists(lists)
    if raw is None:
        raw = eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)[0]
    E.start_run(raw)
    E.compare_own_orientations(p0, E.nMaps if p1 is None else p1)
    E.finish_run(raw)
    pmap = raw[:E.nMaps * 40].view(eng.PROB_MAP_DTYPE)
    pang = raw[E.nMaps * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(E.nAngles, E.nMaps) if E.pd.writeAngles else None
    return raw, pmap, pang


def oracle_ragged(W, E, pd, lists, sel, algo, angles=False):
    """particle p of `sel` (non-empty lists) alone against lists[p] through the CPU oracle, with the constant of the
    handle's volume element: [(prob entry, angle table [K_p] or None)], log P constant"""
    rsel, ssel, s2sel = assert_device_particles_match(E, W.maps, sel)
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(pd, f))
    pts = np.zeros(len(W.points), dtype=orc.POINT_DTYPE)
    for k in ("pos", "radius", "density"):
        pts[k] = W.points[k]
    L = orc.lib()
    out = []
    for i, p in enumerate(sel):
        K = len(lists[p])
        assert K >= 1
        opd.writeAngles = K if angles else 0
        want = np.zeros(1, dtype=orc.PROB_MAP_DTYPE)
        wang = np.zeros((K, 1), dtype=orc.PROB_ANGLE_DTYPE) if angles else None
        ang = np.ascontiguousarray(lists[p], dtype=np.float32)
        L.orc_init_prob(1, K, int(opd.writeAngles), want.ctypes.data, wang.ctypes.data if angles else None)
        L.orc_run(C.byref(opd), algo, pts.ctypes.data, len(pts), W.NormDen, ang.ctypes.data, K, 1, W.px, 0, 0, W.nCTF,
                  W.refCTF.ctypes.data, W.ctfParam.ctypes.data, 1, rsel[i:i + 1].ctypes.data, ssel[i:i + 1].ctypes.data,
                  s2sel[i:i + 1].ctypes.data, 0, K, want.ctypes.data, wang.ctypes.data if angles else None)
        out.append((want[0], wang[:, 0] if angles else None))
    opd.writeAngles = 0
    return out, orc.logp_constant(opd)


def fresh_block(E):
    import bioem_amd.engine as eng
    return eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)[0]


# ------------------------------------------------------------------------------------------------------
# 1. ragged lists against the oracle
# ------------------------------------------------------------------------------------------------------
RAGGED_SHAPES = [
    # N, maxD, single launch, what the shape is there for
    (224, 10, True, "two_column_blocks"),
    (128, 10, True, "nyquist_split"),
    (160, 10, True, "split_last_block"),
    (64, 5, True, "nyquist_column_apart_11_rows"),
    (100, 10, True, "mixed_radix"),
    (224, 13, False, "fastm_per_particle"),
    (75, 10, False, "oddfft_per_particle"),
]


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N,maxD,single,what", RAGGED_SHAPES, ids=[s[3] for s in RAGGED_SHAPES])
def test_ragged_lists_against_oracle(N, maxD, single, what, algo):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=len(LENGTHS), nOrient=27, nEnv=3, maxD=maxD, algo=algo, npts=150)
    try:
        E = W.engine
        assert W.nCTF == 3  # rows per particle are no multiples of four
        assert E.own_kernel_signature == "per particle: " + E.kernel_signature  # the default of every handle
        E.set_own_launch("batch")
        own = E.own_kernel_signature
        if single:
            assert own == E.kernel_signature.replace("k_compare_fast<", "k_compare_fast_own<") and "_own<" in own
        else:
            assert own == "per particle: " + E.kernel_signature
        lists = ragged_lists(W, LENGTHS)
        sel = [p for p, n in enumerate(LENGTHS) if n]
        want, const = oracle_ragged(W, E, W.pd, lists, sel, algo)
        _, got, _ = run_ragged(E, lists)
        assert_round2_matches(got, want, const, sel)
        init = fresh_block(E).view(eng.PROB_MAP_DTYPE)
        for p, n in enumerate(LENGTHS):
            if n == 0:
                assert got[p].tobytes() == init[p].tobytes()  # the empty list's entry is what start_run left
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 2. every own instantiation
# ------------------------------------------------------------------------------------------------------
def _smallest_shape_per_fast_kernel():
    best = {}
    with gzip.open(os.path.join(ROOT, "tests", "golden", "selection_snapshot.txt.gz"), "rt") as f:
        for ln in f:
            N, d, g, algo, sig = ln.rstrip("\n").split(" ", 4)
            if not sig.startswith("k_compare_fast<") or " x " in sig:
                continue
            cost = (int(N) ** 2 * (2 * (int(d) // int(g)) + 1), int(algo))
            if sig not in best or cost < best[sig][0]:
                best[sig] = (cost, (int(N), int(d), int(g), int(algo), sig))
    return [v[1] for _, v in sorted(best.items())]


@pytest.mark.parametrize("shape", _smallest_shape_per_fast_kernel(), ids=lambda s: s[4].replace(" ", ""))
def test_own_instantiation_against_oracle(shape):
    from bioem_amd.synthetic import Workload
    N, d, g, algo, sig = shape
    W = Workload(N=N, nP=3, nOrient=5, nEnv=2, maxD=d, grid=g, algo=algo, npts=150)
    try:
        E = W.engine
        assert E.kernel_signature == sig
        E.set_own_launch("batch")
        assert E.own_kernel_signature == sig.replace("k_compare_fast<", "k_compare_fast_own<")
        lists = ragged_lists(W, (2, 5, 1))
        want, const = oracle_ragged(W, E, W.pd, lists, [0, 1, 2], algo)
        _, got, _ = run_ragged(E, lists)
        assert_round2_matches(got, want, const, [0, 1, 2])
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 3. one launch per batch == one launch per particle; 4. the two uploads
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["batch", "rows"])
@pytest.mark.parametrize("N", [224, 128, 160])
def test_single_launch_equals_per_particle_launches(N, order):
    """the handle that compares a batch in one launch (block table with a particle's blocks on one XCD, or in row order)
    against a handle set to one launch per particle (Engine.set_own_launch)"""
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=len(LENGTHS), nOrient=27, nEnv=3, npts=150)
    try:
        E = W.engine
        E.set_own_launch(order)
        assert E.own_kernel_signature.startswith("k_compare_fast_own<")
        lists = ragged_lists(W, LENGTHS)
        raw1, _, _ = run_ragged(E, lists, launch=order)
        raw2, _, _ = run_ragged(E, lists, upload=False)
        assert raw1.tobytes() == raw2.tobytes()  # a rerun: no atomics, no races
        E2, _ = plain_engine(W, 27, 1)
        try:
            E2.set_own_launch("particle")
            assert E2.own_kernel_signature == "per particle: " + E2.kernel_signature
            raw3, _, _ = run_ragged(E2, lists, launch="particle")
            assert E2.own_kernel_signature == "per particle: " + E2.kernel_signature
            assert raw3.tobytes() == raw1.tobytes()
        finally:
            E2.close()
        # and the mode of a handle may change between passes without a new upload
        E.set_own_launch("particle")
        assert E.own_kernel_signature == "per particle: " + E.kernel_signature
        raw4, _, _ = run_ragged(E, lists, upload=False)
        E.set_own_launch("batch")
        raw5, _, _ = run_ragged(E, lists, upload=False)
        assert raw4.tobytes() == raw1.tobytes() and raw5.tobytes() == raw1.tobytes()
        assert E.L.bioem_hip_set_own_launch(E.h, 7) == 2
    finally:
        W.engine.close()


def test_uniform_lists_through_both_uploads():
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=7, nOrient=5, nEnv=3, npts=150)
    try:
        E = W.engine
        lists = random_lists(W, 5)
        raw_old, _, _ = run_own(E, lists)
        raw_new, _, _ = run_ragged(E, [lists[p] for p in range(W.nP)])
        assert raw_new.tobytes() == raw_old.tobytes()
        flat = lists.reshape(-1, 4)
        raw_flat, _, _ = run_ragged(E, (flat, np.arange(W.nP + 1, dtype=np.int64) * 5))
        assert raw_flat.tobytes() == raw_old.tobytes()
    finally:
        W.engine.close()


def test_two_lists_in_a_tuple_are_not_taken_for_flat_and_offsets():
    """a tuple of two per-particle lists, the second one quaternion given as a flat 4-vector, is two lists: (flat,
    offsets) needs nMaps + 1 integers"""
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=2, nOrient=5, nEnv=2, npts=150)
    try:
        E = W.engine
        lists = random_lists(W, 3)
        raw_list, _, _ = run_ragged(E, [lists[0], lists[1, :1]])
        raw_tuple, pmap, _ = run_ragged(E, (lists[0], lists[1, 0]))
        assert raw_tuple.tobytes() == raw_list.tobytes()
        raw_int, _, _ = run_ragged(E, (lists[0], [0, 0, 0, 1]))  # the identity, written in integers
        assert raw_int.tobytes() == run_ragged(E, [lists[0], np.array([[0, 0, 0, 1]], dtype=np.float32)])[0].tobytes()
        raw_flat, _, _ = run_ragged(E, (lists.reshape(-1, 4)[:4], [0, 3, 4]))
        assert raw_flat.tobytes() == raw_list.tobytes()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 5. many particles per batch
# ------------------------------------------------------------------------------------------------------
def test_many_particles_per_batch():
    from bioem_amd.synthetic import Workload
    nP = 300
    lengths = [1 + p % 9 for p in range(nP)]
    W = Workload(N=64, nP=nP, nOrient=9, nEnv=2, npts=150)
    try:
        E = W.engine
        E.set_own_launch("batch")
        assert E.own_kernel_signature.startswith("k_compare_fast_own<")
        lists = ragged_lists(W, lengths)
        sel = [0, 8, 9, 77, 150, 151, 298, 299]
        want, const = oracle_ragged(W, E, W.pd, lists, sel, 1)
        E.set_phase_timing(True)
        raw1, got, _ = run_ragged(E, lists)
        rec = E.phase_records()
        E.set_phase_timing(False)
        cmp_rec = rec[rec["phase"] == 2]
        assert len(cmp_rec) >= 2 and cmp_rec["iOrientEnd"][-1] == sum(lengths)
        assert (cmp_rec["iOrientEnd"] - cmp_rec["iOrientBegin"]).max() >= 64  # dozens of particles in one launch
        assert_round2_matches(got, want, const, sel)
        E2, _ = plain_engine(W, 9, 1)
        try:
            E2.set_own_launch("particle")
            raw2, _, _ = run_ragged(E2, lists, launch="particle")
            assert raw2.tobytes() == raw1.tobytes()
        finally:
            E2.close()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 6. a long list across batch boundaries
# ------------------------------------------------------------------------------------------------------
def test_long_list_straddles_batches():
    """183 slots in batches of 64 (the phase records say so): the 150-entry list of particle 2 begins in the first batch
    and ends in the third"""
    from bioem_amd.synthetic import Workload
    lengths = [3, 5, 150, 2, 7, 1, 4, 6, 2, 3]
    W = Workload(N=64, nP=len(lengths), nOrient=150, nEnv=2, npts=150)
    try:
        E = W.engine
        lists = ragged_lists(W, lengths)
        sel = list(range(W.nP))
        want, const = oracle_ragged(W, E, W.pd, lists, sel, 1)
        E.set_phase_timing(True)
        _, got, _ = run_ragged(E, lists)
        rec = E.phase_records()
        E.set_phase_timing(False)
        cmp_rec = rec[rec["phase"] == 2]
        assert len(cmp_rec) >= 2 and cmp_rec["iOrientBegin"][0] == 0 and cmp_rec["iOrientEnd"][-1] == sum(lengths)
        assert np.array_equal(cmp_rec["iOrientBegin"][1:], cmp_rec["iOrientEnd"][:-1])
        lo, hi = sum(lengths[:2]), sum(lengths[:3])
        assert any(lo < b < hi for b in cmp_rec["iOrientBegin"][1:]), "the long list straddles no batch boundary"
        assert_round2_matches(got, want, const, sel)
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 7. angle table; 8. particle range
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 2])
def test_angle_table_with_ragged_lists(algo):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=len(LENGTHS), nOrient=27, nEnv=3, algo=algo, npts=150)
    try:
        E, pd = plain_engine(W, 27, algo, write_angles=27)
        try:
            lists = ragged_lists(W, LENGTHS)
            sel = [p for p, n in enumerate(LENGTHS) if n]
            want, const = oracle_ragged(W, E, pd, lists, sel, algo, angles=True)
            _, got, pang = run_ragged(E, lists)
            assert_round2_matches(got, want, const, sel)
            ainit = fresh_block(E)[W.nP * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(27, W.nP)
            with np.errstate(divide="ignore"):
                dev = np.log(pang["forAngles"]) + pang["ConstAngle"]  # [k][p]
            for p, n in enumerate(LENGTHS):
                assert pang[n:, p].tobytes() == ainit[n:, p].tobytes()  # entries at or above K_p are untouched
            for p, (_, wa) in zip(sel, want):
                ref = np.log(wa["forAngles"]) + wa["ConstAngle"]
                n = LENGTHS[p]
                print("particle %d: max table diff %.3g" % (p, np.abs(dev[:n, p] - ref).max()))
                assert np.abs(dev[:n, p] - ref).max() <= ABS_TOL
            top = E.topk_angles(5, const)
            for p, n in enumerate(LENGTHS):
                m = min(5, n)  # (beyond the list the table holds equal, untouched entries)
                order = sorted(range(n), key=lambda k: (dev[k, p], k), reverse=True)[:m]
                assert list(top[p]["orient"][:m]) == order
                assert np.array_equal(top[p]["logp"][:m],
                                      np.log(pang["forAngles"][order, p]) + pang["ConstAngle"][order, p] + const)
        finally:
            E.close()
    finally:
        W.engine.close()


def test_particle_range_with_ragged_lists():
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    lengths = [4, 1, 9, 2, 0, 27, 3, 5, 1, 6]
    W = Workload(N=64, nP=10, nOrient=27, nEnv=2, npts=150, write_angles=0)
    try:
        E, pd = plain_engine(W, 27, 1, write_angles=27)
        try:
            lists = ragged_lists(W, lengths)
            fresh = fresh_block(E)
            _, got, pang = run_ragged(E, lists, 3, 7)
            want, const = oracle_ragged(W, E, pd, lists, [3, 5, 6], 1)
            assert_round2_matches(got, want, const, [3, 5, 6])
            init = fresh[:W.nP * 40].view(eng.PROB_MAP_DTYPE)
            ainit = fresh[W.nP * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(27, W.nP)
            for p in (0, 1, 2, 4, 7, 8, 9):
                assert got[p].tobytes() == init[p].tobytes()
                assert pang[:, p].tobytes() == ainit[:, p].tobytes()
            for p in (3, 5, 6):
                assert np.all(pang[:lengths[p], p]["forAngles"] > 0.0)
        finally:
            E.close()
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 9. refusals
# ------------------------------------------------------------------------------------------------------
def test_refused_offsets_leave_the_handle_usable():
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=3, nOrient=8, nEnv=2, npts=150)
    try:
        E = W.engine
        flat = np.ascontiguousarray(random_lists(W, 9).reshape(-1, 4))

        def refused(offsets, message):
            off = np.asarray(offsets, dtype=np.int64)
            rc = E.L.bioem_hip_upload_particle_orientation_lists(E.h, flat.ctypes.data_as(C.c_void_p),
                                                                 off.ctypes.data_as(C.c_void_p), 1)
            assert rc == 2
            assert message in E.L.bioem_hip_last_error(E.h).decode()
            raw = eng.new_prob_block(W.nP, E.nAngles, 0)[0]
            E.start_run(raw)
            E.project_convolve_compare(0, W.nOrient)
            E.finish_run(raw)
            assert np.all(raw[:W.nP * 40].view(eng.PROB_MAP_DTYPE)["Total"] > 0.0)

        refused([1, 3, 5, 8], "offsets[0] must be 0")
        refused([0, 5, 3, 8], "offsets must not decrease")
        refused([0, 9, 10, 12], "a list is longer than nAngles")
        refused([0, 0, 0, 0], "the lists are all empty")
        # and a good upload after the refusals runs
        lists = ragged_lists(W, (2, 0, 8))
        want, const = oracle_ragged(W, E, W.pd, lists, [0, 2], 1)
        _, got, _ = run_ragged(E, lists)
        assert_round2_matches(got, want, const, [0, 2])
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# 10. command line: --RefineSeeds / --RefineLogWindow
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,algo", [("g2_n128", 2), ("g10_n64", 1)])
def test_cli_refine_seeds(name, algo, tmp_path):
    """--RefineSeeds 1 writes the files of a run without it; with --RefineSeeds 3 --RefineLogWindow 5 OutputFile is
    unchanged, no ANG_PROB appears, and every particle of OutputFile_Round2 is what this CLI prints for that particle
    alone with its concatenated list through --ReadOrientation.  The seeds are taken from the CPU oracle's angle table
    of round 1 (refine.seed_lists on its three best per particle): with a window of 5 the particles of both cases get
    lists of 1, 2 and 3 seeds, and no candidate lies closer than 0.07 to the window's edge."""
    import subprocess

    import io_formats as iof
    from bioem_amd import refine
    from bioem_amd.engine import CANDIDATE_DTYPE
    from golden_util import load_case, oracle_setup, write_case_inputs
    from test_gpu_parity import REL_TOL
    from test_own_lists import STEP, _write_quaternions
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
    G = len(grid)
    run(inputs + ["--OutputFile", "plain.txt", "--RefineOrientations", "grid.txt"])
    run(inputs + ["--OutputFile", "one.txt", "--RefineOrientations", "grid.txt", "--RefineSeeds", "1"])
    for suffix in ("", "_Round2"):
        assert open(d / ("one.txt" + suffix), "rb").read() == open(d / ("plain.txt" + suffix), "rb").read()
    run(inputs + ["--OutputFile", "out.txt", "--RefineOrientations", "grid.txt", "--RefineSeeds", "3", "--RefineLogWindow",
                  "5"])
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    assert not os.path.exists(d / "ANG_PROB")
    r2 = iof.parse_output_probabilities(open(d / "out.txt_Round2").read())
    angles = np.array([[np.float32(float(ln[12 * c:12 * c + 12])) for c in range(4)] for ln in case["orient_lines"]],
                      dtype=np.float32)
    nP = len(case["maps"])
    assert len(r2) == nP
    # the seeds: the oracle's ranking of round 1
    S = oracle_setup(case)
    S.pd.writeAngles = 3
    _, pa = S.run(algo)
    lp = np.log(pa["forAngles"]) + pa["ConstAngle"]  # [nAngles][nMaps]
    cands = np.zeros((nP, 3), dtype=CANDIDATE_DTYPE)
    for p in range(nP):
        order = sorted(range(S.nAngles), key=lambda o: (lp[o, p], o), reverse=True)[:3]
        cands[p]["orient"] = order
        cands[p]["logp"] = lp[order, p]
        gaps = lp[order[0], p] - lp[order[1:], p]
        assert np.all(np.abs(gaps - 5.0) > 0.05)  # nobody sits on the window's edge
    flat, off = refine.seed_lists(angles, cands, grid, max_seeds=3, log_window=5.0)
    lengths = np.diff(off)
    print("seeds per particle:", list(lengths // G))
    assert len(set(lengths)) > 1, "every particle got the same list length"
    margs = inputs[:inputs.index("--Particlesfile")]
    for p in range(nP):
        lst = flat[off[p]:off[p + 1]]
        _write_quaternions(d / ("list%d.txt" % p), lst)
        iof.write_text_particles(os.path.join(str(d), "one%d.txt" % p), case["maps"][p:p + 1])
        run(margs + ["--Particlesfile", "one%d.txt" % p, "--ReadOrientation", "list%d.txt" % p, "--OutputFile",
                     "single%d.txt" % p])
        s = iof.parse_output_probabilities(open(d / ("single%d.txt" % p)).read())[0]
        m = r2[p]
        print("particle %d: %d entries, round 2 %.4f alone %.4f" % (p, len(lst), m["logp"], s["logp"]))
        assert abs(m["logp"] - s["logp"]) <= REL_TOL * abs(s["logp"])
        assert abs(m["logp"] - s["logp"]) <= max(ABS_TOL, 2.0 * float(np.spacing(np.float32(abs(s["logp"])))))
        assert (m["angles"], m["ctf"], m["cx"], m["cy"]) == (s["angles"], s["ctf"], s["cx"], s["cy"])
        assert abs(m["norm"] - s["norm"]) <= 1e-4 * max(1.0, abs(s["norm"]))
        assert abs(m["mu"] - s["mu"]) <= 1e-4 * max(1.0, abs(s["mu"]))
