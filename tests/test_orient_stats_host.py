"""Host side of the orientation-posterior summaries (no GPU): the mpmath reference of the sums and of what is derived from
them (tests/orient_reference.py) on hand-made tables, the ABI exports, the merge of shard sums
(bioem_hip_merge_orient_sums_host) against the reference of the concatenated table, orient_stats.derive on planted cases,
the 4 x 4 Jacobi solver of the CLI against numpy's eigh, and the --OrientStats writer and parser."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

import orient_reference as R

U = 2.0 ** -53


def quat_about(axis, deg):
    """unit quaternion (x, y, z, w) of a rotation by deg about axis"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(deg) / 2.0
    return np.array([a[0] * math.sin(h), a[1] * math.sin(h), a[2] * math.sin(h), math.cos(h)])


def record(ref, **kw):
    import bioem_amd.engine as eng
    return R.as_record(ref, eng.ORIENT_SUMS_DTYPE, **kw)


# ------------------------------------------------------------------------------------------------------
# the reference on hand-made tables
# ------------------------------------------------------------------------------------------------------
def test_reference_closed_forms():
    # three entries with F e^C = 1, 2, 1 (times e^-5), one never compared
    F = [1.0, 2.0, 0.0, 1.0]
    C = [-5.0, -5.0, 77.0, -5.0]
    r = R.sums(F, C)
    assert (r.omax, r.count) == (1, 3)
    with mpmath.workprec(R.PREC):
        ln2 = mpmath.log(2)
        assert abs(r.m - (ln2 - 5)) < 1e-70
        assert abs(r.S0 - 2) < 1e-70 and abs(r.S2 - mpmath.mpf(3) / 2) < 1e-70 and abs(r.S1 + ln2) < 1e-70
        s = R.derive(r)
        assert abs(s.logZ - (mpmath.log(4) - 5)) < 1e-70 and abs(s.pTop - mpmath.mpf(1) / 2) < 1e-70
        assert abs(s.entropy - mpmath.log(8) / 2) < 1e-70            # p = 1/4, 1/2, 1/4
        assert abs(s.nEff - mpmath.mpf(8) / 3) < 1e-70
    assert s.mean is None
    # the lowest index keeps a tie; a prior moves the maximum; sums relative to a given m
    assert R.sums([3.0, 1.0, 3.0], [5.0, 5.0, 5.0]).omax == 0
    assert R.sums([1.0, 1.0], [0.0, 0.0], prior=[0.0, 0.5]).omax == 1
    a, b = R.sums(F, C), R.sums(F, C, m=3.0)
    with mpmath.workprec(R.PREC):
        assert abs(R.derive(a).logZ - R.derive(b).logZ) < 1e-70 and abs(R.derive(a).entropy - R.derive(b).entropy) < 1e-70
    # nothing compared
    e = R.sums([0.0, 0.0], [R.MIN_PROB, R.MIN_PROB])
    assert (e.omax, e.count, float(e.m)) == (-1, 0, R.MIN_PROB) and e.S0 == 0


def test_reference_moments_do_not_see_the_sign_or_the_length_of_a_quaternion():
    rng = np.random.default_rng(3)
    q = rng.standard_normal((7, 4)).astype(np.float32)
    F, Cc = rng.uniform(0.5, 2.0, 7), rng.uniform(-3, 3, 7)
    a = R.sums(F, Cc, quats=q)
    q2 = q.copy()
    q2[::2] *= -1
    q2[1] *= 4                                        # (exact in float)
    b = R.sums(F, Cc, quats=q2)
    assert a.Q == b.Q
    with mpmath.workprec(R.PREC):
        assert abs(a.Q[0] + a.Q[4] + a.Q[7] + a.Q[9] - a.S0) < 1e-55          # trace of q q^T = 1


# ------------------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------------------
def test_abi_exports():
    import bioem_amd.engine as eng
    L = eng.load_library()
    for f in ("bioem_hip_orientation_sums", "bioem_hip_merge_orient_sums_host", "bioem_hip_debug_orient_sums",
              "bioem_hip_debug_orient_sums_own"):
        assert hasattr(L, f), f
        assert f in eng.EXPORTS
    assert eng.ORIENT_SUMS_DTYPE.itemsize == 136
    assert hasattr(eng.Engine, "orientation_sums") and hasattr(eng, "merge_orient_sums")
    from bioem_amd import hostlib
    H = hostlib.load_host_library()
    assert hasattr(H, "bioem_host_write_orient_stats") and hasattr(H, "bioem_host_jacobi4")
    # the merge refuses what it cannot take
    out = np.zeros(1, dtype=eng.ORIENT_SUMS_DTYPE)
    assert L.bioem_hip_merge_orient_sums_host(0, 1, None, out.ctypes.data_as(C.c_void_p)) == 2
    arr = (C.c_void_p * 1)(out.ctypes.data)
    assert L.bioem_hip_merge_orient_sums_host(1, 1, arr, None) == 2


# ------------------------------------------------------------------------------------------------------
# merge of shard sums against the reference of the concatenated table
# ------------------------------------------------------------------------------------------------------
def merge_table(seed, nO=40, nP=6):
    rng = np.random.default_rng(seed)
    F = rng.uniform(0.2, 5.0, (nO, nP))
    Cc = rng.uniform(-40.0, 30.0, (nO, nP)) + rng.uniform(-800, 400, nP)[None, :]
    F[rng.random((nO, nP)) < 0.1] = 0.0
    q = rng.standard_normal((nO, 4)).astype(np.float32)
    return F, Cc, q


def shard_records(F, Cc, q, cuts):
    """per shard [nP] records: the reference of the shard's rows relative to the double nearest its own maximum"""
    import bioem_amd.engine as eng
    out = []
    for o0, o1 in cuts:
        rec = np.zeros(F.shape[1], dtype=eng.ORIENT_SUMS_DTYPE)
        for p in range(F.shape[1]):
            top = R.sums(F[o0:o1, p], Cc[o0:o1, p], quats=q[o0:o1])
            if top.count:
                top = R.sums(F[o0:o1, p], Cc[o0:o1, p], quats=q[o0:o1], m=float(top.m))
            rec[p] = record(top, omax_offset=o0, has_moments=1)
        out.append(rec)
    return out


def assert_merge_matches(merged, F, Cc, q, nShards):
    for p in range(F.shape[1]):
        g = merged[p]
        ref = R.sums(F[:, p], Cc[:, p], quats=q, m=float(g["m"]))
        assert (int(g["omax"]), int(g["count"])) == (ref.omax, ref.count), p
        if not ref.count:
            assert g["m"] == R.MIN_PROB and g["S0"] == 0 and not g["Q"].any()
            continue
        # the shard sums enter rounded to double (1 u), are scaled by an exp (2 u) of a difference of doubles (|d| u;
        # |d| <= 2 A), multiplied (1 u) and added (nShards u): first order (2 A + 4 + nShards) u, doubled; S2 twice the
        # exponent's part, S1 on the scale sum e^d (|d| + 1)
        A = float(ref.A)
        c1, c2 = 2 * (2 * A + 4 + nShards) * U, 2 * (4 * A + 4 + nShards) * U
        assert abs(float(g["m"]) - float(ref.m)) <= float(ref.mbound) + abs(float(ref.m)) * U
        for f, c in (("S0", c1), ("S1", c1), ("S2", c2)):
            err, lim = abs(mpmath.mpf(float(g[f])) - getattr(ref, f)), c * ref.scale[f]
            assert err <= lim, (p, f, float(err), float(lim))
        for k in range(10):
            assert abs(mpmath.mpf(float(g["Q"][k])) - ref.Q[k]) <= c1 * ref.scale["Q"][k], (p, k)


@pytest.mark.parametrize("cuts", [[(0, 40)], [(0, 13), (13, 14), (14, 40)]], ids=["1_shard", "3_shards"])
def test_merge_against_the_concatenated_table(cuts):
    import bioem_amd.engine as eng
    F, Cc, q = merge_table(11)
    merged = eng.merge_orient_sums(shard_records(F, Cc, q, cuts))
    assert_merge_matches(merged, F, Cc, q, len(cuts))
    if len(cuts) == 1:
        assert merged.tobytes() == shard_records(F, Cc, q, cuts)[0].tobytes()


def test_merge_with_an_empty_shard_and_equal_maxima():
    import bioem_amd.engine as eng
    F, Cc, q = merge_table(12, nO=30, nP=4)
    F[10:20, :] = 0.0                                           # the middle shard compared nothing
    F[:, 3] = 0.0                                               # a particle nobody compared
    # particle 0: the same entry bits at the top of shard 0 and of shard 2 -> the lowest index keeps the tie
    F[4, 0], Cc[4, 0] = 1.5, 900.0
    F[25, 0], Cc[25, 0] = 1.5, 900.0
    cuts = [(0, 10), (10, 20), (20, 30)]
    recs = shard_records(F, Cc, q, cuts)
    assert recs[1]["count"].sum() == 0 and np.all(recs[1]["omax"] == -1)
    assert recs[0]["m"][0] == recs[2]["m"][0]
    merged = eng.merge_orient_sums(recs)
    assert int(merged["omax"][0]) == 4
    assert merged["count"][3] == 0 and merged["omax"][3] == -1 and merged["m"][3] == R.MIN_PROB
    assert_merge_matches(merged, F, Cc, q, 3)
    # the other order of the tie: a later shard wins only when strictly greater
    assert int(eng.merge_orient_sums([recs[2], recs[1], recs[0]])["omax"][0]) == 25


# ------------------------------------------------------------------------------------------------------
# derive on planted cases
# ------------------------------------------------------------------------------------------------------
def derived(F, Cc, quats, prior=None):
    from bioem_amd import orient_stats
    ref = R.sums(F, Cc, prior=prior, quats=quats)
    rec = record(ref, has_moments=quats is not None)
    return orient_stats.derive(rec, None if quats is None else np.asarray(quats, dtype=np.float32))[0], ref


def test_derive_one_entry():
    q = np.array([quat_about((1, 2, 3), 40.0), quat_about((0, 0, 1), 10.0)], dtype=np.float32)
    s, _ = derived([0.0, 2.5], [R.MIN_PROB, -31.0], q)
    assert s["count"] == 1 and s["omax"] == 1
    assert abs(s["entropy"]) <= 1e-15 and abs(s["nEff"] - 1) <= 1e-15 and abs(s["pTop"] - 1) <= 1e-15
    assert abs(s["logZ"] - (math.log(2.5) - 31.0)) <= 1e-14
    qn = q[1].astype(np.float64) / np.linalg.norm(q[1].astype(np.float64))
    assert np.abs(s["mean"] - qn).max() <= 1e-12 and s["hasMean"] == 1
    assert s["spreadDeg"] <= 1e-5            # acos at 1: the square root of the rounding of lambda


def test_derive_equal_entries():
    nO = 37
    s, _ = derived([1.25] * nO, [-7.0] * nO, None)
    assert abs(s["entropy"] - math.log(nO)) <= 1e-14 and abs(s["nEff"] - nO) <= 1e-12 and abs(s["pTop"] - 1.0 / nO) <= 1e-16
    assert s["omax"] == 0 and s["hasMean"] == 0


def test_derive_does_not_see_the_sign_of_a_quaternion():
    rng = np.random.default_rng(5)
    q = np.array([quat_about(rng.standard_normal(3), d) for d in rng.uniform(0, 25, 12)], dtype=np.float32)
    F, Cc = rng.uniform(0.5, 2.0, 12), rng.uniform(-2, 2, 12)
    a, ra = derived(F, Cc, q)
    q2 = q.copy()
    q2[1::2] *= -1
    b, rb = derived(F, Cc, q2)
    assert ra.Q == rb.Q
    for f in ("logZ", "entropy", "nEff", "spreadDeg", "pTop"):
        assert a[f] == b[f], f
    sign = 1.0 if a["omax"] % 2 == 0 else -1.0        # the mean follows the arg-max quaternion's sign
    assert np.array_equal(b["mean"], sign * a["mean"])
    # and against the exact eigenvector
    ex = R.derive(ra, q[a["omax"]])
    assert np.abs(a["mean"] - np.array([float(x) for x in ex.mean])).max() <= 1e-12
    assert abs(a["spreadDeg"] - float(ex.spreadDeg)) <= 1e-9


def test_derive_two_quaternions_ten_degrees_apart():
    axis = (0.3, -0.5, 0.8)
    q = np.array([quat_about(axis, 20.0), quat_about(axis, 30.0)])
    s, _ = derived([1.0, 1.0], [3.0, 3.0], q)
    # (float storage of the quaternions: 6e-8 per component)
    assert np.abs(s["mean"] - quat_about(axis, 25.0)).max() <= 2e-7
    assert abs(s["spreadDeg"] - 5.0) <= 1e-5
    assert abs(s["nEff"] - 2) <= 1e-15 and abs(s["entropy"] - math.log(2)) <= 1e-15


def test_suggest_seeds():
    from bioem_amd import orient_stats
    st = np.zeros(6, dtype=orient_stats.STATS_DTYPE)
    st["count"] = [3, 9, 100, 0, 4, 7]
    st["nEff"] = [1.0, 2.000001, 57.3, 0.0, 3.0, 2.0000000005]         # (the last: M >= nEff holds to the last bit)
    assert list(orient_stats.suggest_seeds(st)) == [1, 3, 58, 0, 3, 3]
    assert list(orient_stats.suggest_seeds(st, 0.5)) == [1, 2, 29, 0, 2, 2]
    for M, n in zip(orient_stats.suggest_seeds(st), st["nEff"]):
        assert M >= n and (M - 1 < n or M <= 1)              # the smallest such M
    with pytest.raises(ValueError):
        orient_stats.suggest_seeds(st, 0.0)


# ------------------------------------------------------------------------------------------------------
# the C++ solver
# ------------------------------------------------------------------------------------------------------
def test_jacobi_against_eigh():
    from bioem_amd import hostlib
    rng = np.random.default_rng(9)
    mats = [rng.standard_normal((4, 4)) for _ in range(200)]
    mats = [a + a.T for a in mats]
    v0 = rng.standard_normal((4, 4))
    mats.append(v0 @ np.diag([1e-9, 1.0, 1.0 + 1e-3, 0.25]) @ np.linalg.inv(v0))      # (made symmetric below)
    mats[-1] = (mats[-1] + mats[-1].T) / 2
    mats += [np.diag([0.2, 0.9, 0.4, 0.1]), np.zeros((4, 4)), np.outer(v0[0], v0[0])]
    for A in mats:
        w, v = hostlib.jacobi4(A)
        we, ve = np.linalg.eigh(A)
        scale = max(1e-300, np.abs(A).max())
        assert np.all(np.diff(w) <= 0)
        assert np.abs(w - we[::-1]).max() <= 1e-14 * scale * 4
        assert np.abs(v @ v.T - np.eye(4)).max() <= 1e-14                       # rows orthonormal
        assert np.abs(A @ v.T - v.T * w[None, :]).max() <= 1e-14 * scale * 8    # A v_k = w_k v_k
        gaps = np.abs(np.subtract.outer(we, we))[~np.eye(4, dtype=bool)].min()
        if gaps > 1e-3 * scale:
            for k in range(4):
                assert abs(abs(v[k] @ ve[:, 3 - k]) - 1) <= 1e-11


# ------------------------------------------------------------------------------------------------------
# writer and parser
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("isquat", [True, False], ids=["quaternions", "euler"])
def test_file_round_trip(isquat, tmp_path):
    import bioem_amd.engine as eng
    from bioem_amd import hostlib, orient_stats
    rng = np.random.default_rng(21)
    nO, nP = 19, 5
    F = rng.uniform(0.2, 5.0, (nO, nP))
    Cc = rng.uniform(-6.0, 3.0, (nO, nP)) + rng.uniform(-800, 400, nP)[None, :]
    F[:, 2] = 0.0                                     # a particle that was never compared
    ang = rng.standard_normal((nO, 4)).astype(np.float32)
    if not isquat:
        ang[:, 3] = 0
    sums = np.zeros(nP, dtype=eng.ORIENT_SUMS_DTYPE)
    for p in range(nP):
        sums[p] = record(R.sums(F[:, p], Cc[:, p], quats=ang if isquat else None), has_moments=isquat)
    numconst = -1458.886321
    path = str(tmp_path / "ORIENT_STATS")
    hostlib.write_orient_stats(path, sums, ang, isquat, numconst)
    got, nc, note = orient_stats.parse(path)
    assert nc == numconst and note.startswith(" ORIENT: particle count logZ")
    want = orient_stats.derive(sums, ang, numconst)
    assert len(got) == nP
    for f in ("particle", "count", "omax", "hasMean"):
        assert np.array_equal(got[f], want[f]), f
    assert got["count"][2] == 0 and got["omax"][2] == -1 and got["logZ"][2] == -np.inf and got["hasMean"][2] == 0
    ok = want["count"] > 0
    nA = 4 if isquat else 3
    # (9 significant digits name a float)
    assert np.array_equal(got["angles"][ok, :nA].astype(np.float32), want["angles"][ok, :nA].astype(np.float32))
    for f in ("logZ", "pTop", "entropy", "nEff"):             # 16 significant digits, the solver aside
        assert np.all(np.abs(got[f][ok] - want[f][ok]) <= 4e-15 * np.maximum(1e-3, np.abs(want[f][ok]))), f
    if isquat:
        # Jacobi in the writer, eigh in derive: eigenvectors to 1e-12, the spread through acos(sqrt(lambda))
        assert np.abs(got["mean"][ok] - want["mean"][ok]).max() <= 1e-12
        assert np.abs(got["spreadDeg"][ok] - want["spreadDeg"][ok]).max() <= 1e-9
        assert np.all((got["mean"][ok] * ang[want["omax"][ok]]).sum(1) >= 0)
    else:
        assert not got["hasMean"].any()
        assert open(path).read().count(" - -\n") == nP
    # a malformed file
    bad = tmp_path / "bad"
    bad.write_text(open(path).read().replace("ORIENT 1 ", "ORIENT 1 x ", 1))
    with pytest.raises(ValueError):
        orient_stats.parse(str(bad))
