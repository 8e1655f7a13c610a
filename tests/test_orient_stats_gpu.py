"""Summaries of the orientation posterior, reduced on the device where the angle table lives
(bioem_hip_orientation_sums: k_orient_max, k_orient_sums, k_orient_fold).

1. The kernels alone (bioem_hip_debug_orient_sums) against the mpmath reference (tests/orient_reference.py) on the same
   table bits: count and omax exactly, m within the bound of the device key, every sum within the derived bound
   [c A + 2 (T + 16)] 2^-53 of its own scale (c = 6, for S2 12; the derivation is in the reference
   module's text); table sizes at the chunk edges (256 orientations) and the lane edges (64 particles).
2. The chain on golden cases: the handle's sums equal the kernels run on the table finish_run returned, bit for bit;
   what orient_stats.derive makes of them against the mpmath statistics of the ORACLE's table with the project's
   tolerances (tests/test_gpu_parity.py: REL_TOL relative and ABS_TOL absolute on a log posterior).
3. Shards merged on the host against the unsharded sums: m, omax, count exactly, the sums to 1e-12 (of |S1| + S0 for S1
   and of S0 for Q: those can cancel or vanish, their terms are of that size).
4. Own lists, 5. refusals, 6. the command line."""
import ctypes as C
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

import oracle as orc
import orient_reference as R
from golden_util import write_case_inputs
from test_gpu_parity import ABS_TOL, REL_TOL, make_engine, make_shard_engine, pd_of, run_native, run_shard, setup_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = ("S0", "S1", "S2")


@pytest.fixture(scope="module")
def hook():
    """any handle serves the debug hook: the kernels run on what is handed in"""
    _, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    yield E
    E.close()


# ------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ------------------------------------------------------------------------------------------------------
def make_table(nO, nMaps, seed):
    """entries with ConstAngle in [-900, 500] and forAngles from a pool of 256 values in e^[-7, 7]; per particle a base
    near which three quarters of the entries lie (many terms that count), the rest anywhere down to -900; particle 1 spans
    the whole 1 400 log units; rows 0, nO / 2 and nO - 1 were never compared; the last particle is empty; particle 0 (and
    64) holds the same top entry, bit for bit, in rows 1 and nO - 2"""
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
    ties = {}
    if nO >= 5:
        if nMaps > 1:
            tab["ConstAngle"][3, 1], tab["ConstAngle"][nO - 3, 1] = 500.0, -900.0
        for p in (0, 64):
            if p < nMaps - 1 or (p == 0 and nMaps == 1):
                for r in (1, nO - 2):
                    tab["forAngles"][r, p], tab["ConstAngle"][r, p] = pool[0], 500.0
                ties[p] = 1
        for r in (0, nO // 2, nO - 1):
            tab["forAngles"][r, :], tab["ConstAngle"][r, :] = 0.0, R.MIN_PROB
    if nMaps > 1:
        tab["forAngles"][:, nMaps - 1], tab["ConstAngle"][:, nMaps - 1] = 0.0, R.MIN_PROB
    quats = rng.standard_normal((nO, 4)).astype(np.float32)
    prior = rng.uniform(-2.0, 0.0, nO) if nO in (255, 513) else None
    if prior is not None:
        prior[nO - 2] = prior[1]                    # (a tie is a tie of the keys: the same prior on both rows)
    return tab, quats, prior, ties


def assert_against_reference(got, tab, quats, prior, ties=None, label=""):
    nO, nMaps = tab.shape
    qq = R.products(quats) if quats is not None else None
    worst = dict(m=0.0, S0=0.0, S1=0.0, S2=0.0, Q=0.0)
    for p in range(nMaps):
        g = got[p]
        ref = R.sums(tab["forAngles"][:, p], tab["ConstAngle"][:, p], prior=prior, qq=qq, m=float(g["m"]))
        assert (int(g["count"]), int(g["omax"])) == (ref.count, ref.omax), (p, g["count"], g["omax"], ref.count, ref.omax)
        assert g["hasMoments"] == (1.0 if quats is not None else 0.0)
        if ref.count == 0:
            assert g["m"] == R.MIN_PROB and g["omax"] == -1
            assert g["S0"] == 0 and g["S1"] == 0 and g["S2"] == 0 and not g["Q"].any()
            continue
        if ties and p in ties:
            assert int(g["omax"]) == ties[p]
        with mpmath.workprec(R.PREC):
            em = abs(mpmath.mpf(float(g["m"])) - ref.m)
            assert em <= ref.mbound, (p, float(em), float(ref.mbound))
            worst["m"] = max(worst["m"], float(em / ref.mbound))
            b = R.bounds(ref)
            for f in SUMS:
                err = abs(mpmath.mpf(float(g[f])) - getattr(ref, f))
                assert err <= b[f], (p, f, float(err), float(b[f]))
                worst[f] = max(worst[f], float(err / b[f]))
            for k in range(10):
                err = abs(mpmath.mpf(float(g["Q"][k])) - ref.Q[k])
                assert err <= b["Q"][k], (p, k, float(err), float(b["Q"][k]))
                if b["Q"][k] > 0:
                    worst["Q"] = max(worst["Q"], float(err / b["Q"][k]))
    print("%s%d x %d: worst error / bound  m %.3g  S0 %.3g  S1 %.3g  S2 %.3g  Q %.3g"
          % (label, nO, nMaps, worst["m"], worst["S0"], worst["S1"], worst["S2"], worst["Q"]))


@pytest.mark.parametrize("nMaps", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("nO", [1, 255, 256, 257, 513])
def test_kernels_against_mpmath(hook, nO, nMaps):
    tab, quats, prior, ties = make_table(nO, nMaps, 1000 * nO + nMaps)
    got = hook.debug_orient_sums(tab, quats, True, prior)
    assert_against_reference(got, tab, quats, prior, ties)
    assert hook.debug_orient_sums(tab, quats, True, prior).tobytes() == got.tobytes()        # the same bits on every run


def test_euler_lists_have_no_moments_and_the_same_scalar_sums(hook):
    tab, quats, prior, _ = make_table(257, 65, 7)
    a = hook.debug_orient_sums(tab, quats, True, prior)
    for b in (hook.debug_orient_sums(tab, quats, False, prior), hook.debug_orient_sums(tab, None, True, prior)):
        assert not b["hasMoments"].any() and not b["Q"].any()
        for f in ("m", "omax", "count") + SUMS:
            assert a[f].tobytes() == b[f].tobytes(), f


def test_particle_order_and_table_width_do_not_change_a_particle(hook):
    tab, quats, prior, _ = make_table(513, 130, 8)
    whole = hook.debug_orient_sums(tab, quats, True, prior)
    perm = np.random.default_rng(2).permutation(130)
    assert hook.debug_orient_sums(tab[:, perm], quats, True, prior).tobytes() == whole[perm].tobytes()
    for p0, p1 in ((0, 65), (63, 64), (1, 130)):
        part = hook.debug_orient_sums(np.ascontiguousarray(tab[:, p0:p1]), quats, True, prior)
        assert part.tobytes() == whole[p0:p1].tobytes()


def test_own_list_instantiation_against_the_shared_kernel_per_particle(hook):
    """ragged lists, lengths 0 and nO among them: lane p forms the products of ITS quaternion; every particle must come
    out as the shared kernel gives it for a one-particle table over that particle's list, bit for bit"""
    nO, nMaps = 300, 70
    tab, _, _, _ = make_table(nO, nMaps, 9)
    rng = np.random.default_rng(10)
    lengths = rng.integers(1, nO, nMaps)
    lengths[[0, 5, 64]] = [nO, 0, nO]
    lengths[[6, 65]] = [256, 257]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    flat = rng.standard_normal((int(off[-1]), 4)).astype(np.float32)
    for p in range(nMaps):
        tab["forAngles"][lengths[p]:, p], tab["ConstAngle"][lengths[p]:, p] = 0.0, R.MIN_PROB
    got = hook.debug_orient_sums(tab, flat, True, offsets=off)
    assert got["count"][5] == 0 and got["omax"][5] == -1 and got["count"][nMaps - 1] == 0
    for p in range(nMaps):
        n = int(lengths[p])
        if n == 0:
            assert got[p]["m"] == R.MIN_PROB and got[p]["S0"] == 0
            continue
        one = hook.debug_orient_sums(np.ascontiguousarray(tab[:n, p:p + 1]), flat[off[p]:off[p + 1]], True)
        assert one[0].tobytes() == got[p].tobytes(), p
    # an entry beyond a particle's list does not count, whatever it holds
    stale = tab.copy()
    stale["forAngles"][lengths[7]:, 7], stale["ConstAngle"][lengths[7]:, 7] = 3.0, 499.0
    assert hook.debug_orient_sums(stale, flat, True, offsets=off).tobytes() == got.tobytes()
    with pytest.raises(RuntimeError, match="offsets") as ei:
        hook.debug_orient_sums(tab, flat, True, offsets=off[::-1].copy())
    assert ei.value.rc == 2


# ------------------------------------------------------------------------------------------------------
# 2. the chain
# ------------------------------------------------------------------------------------------------------
def prior_of(S):
    pri = S.P.get("angprior")
    return None if pri is None else np.asarray(pri, dtype=np.float64)


_oracle_stats = {}


def oracle_stats(name, algo):
    """mpmath sums and statistics of the ORACLE's angle table, per particle; computed once"""
    key = (name, algo)
    if key not in _oracle_stats:
        _, S = setup_for(name)
        wm, wa = S.run(algo)
        qq = R.products(S.angles) if S.isQuat else None
        out = []
        for p in range(S.nMaps):
            ref = R.sums(wa["forAngles"][:, p], wa["ConstAngle"][:, p], prior=prior_of(S), qq=qq)
            out.append((ref, R.derive(ref, S.angles[ref.omax] if S.isQuat else None)))
        _oracle_stats[key] = (wm, wa, out)
    return _oracle_stats[key]


@pytest.mark.parametrize("name", ["g4_n32_angles", "g11_n32_eulerlist"])
def test_chain_against_the_oracle(name):
    from bioem_amd import orient_stats
    case, S = setup_for(name)
    prior = prior_of(S)
    assert (prior is not None) == (name == "g11_n32_eulerlist")
    for algo in case["algos"]:
        E = make_engine(S, algo)
        _, pmap, pang = run_native(E, S)
        sums = E.orientation_sums(prior)
        assert sums.shape == (S.nMaps,)
        # the handle's table is the one finish_run returned: the same kernels on it give the same bits
        assert E.debug_orient_sums(pang, S.angles, S.isQuat, prior).tobytes() == sums.tobytes()
        assert E.orientation_sums(prior, 1, S.nMaps).tobytes() == sums[1:].tobytes()          # a sub-range
        assert_against_reference(sums, pang, S.angles if S.isQuat else None, prior, label="%s ALGO %d " % (name, algo))
        # without priors: the log evidence over the orientations is the particle entry's (double rounding only)
        plain = E.orientation_sums()
        logZ = plain["m"] + np.log(plain["S0"])
        entry = np.log(pmap["Total"]) + pmap["Constoadd"]
        print("max |logZ - (log Total + Constoadd)| %.3g" % np.abs(logZ - entry).max())
        assert np.abs(logZ - entry).max() <= 1e-10
        if not S.isQuat:
            assert not sums["hasMoments"].any() and not sums["Q"].any()
        else:
            assert sums["hasMoments"].all()
        E.close()
        wm, wa, want = oracle_stats(name, algo)
        rows = orc.ang_prob_rows(S, wm, wa)
        st = orient_stats.derive(sums, S.angles)
        for p in range(S.nMaps):
            ref, ex = want[p]
            lz, H, nE = float(ex.logZ), float(ex.entropy), float(ex.nEff)
            print("particle %d: logZ %.6f oracle %.6f | H %.6g oracle %.6g (rel %.3g) | nEff %.6g oracle %.6g (rel %.3g)"
                  % (p, st["logZ"][p], lz, st["entropy"][p], H, abs(st["entropy"][p] - H) / abs(H), st["nEff"][p], nE,
                     abs(st["nEff"][p] - nE) / nE))
            assert st["count"][p] == S.nAngles
            assert st["omax"][p] == ref.omax == rows[p][0]["orient"]
            assert abs(st["logZ"][p] - lz) <= REL_TOL * abs(lz) and abs(st["logZ"][p] - lz) <= ABS_TOL
            assert abs(st["pTop"][p] - float(ex.pTop)) <= REL_TOL * float(ex.pTop)
            assert abs(st["entropy"][p] - H) <= REL_TOL * abs(H)
            assert abs(st["nEff"][p] - nE) <= REL_TOL * nE
            if S.isQuat:
                mean = np.array([float(x) for x in ex.mean])
                print("            mean %s oracle %s | spread %.6f oracle %.6f deg"
                      % (st["mean"][p], mean, st["spreadDeg"][p], float(ex.spreadDeg)))
                assert np.abs(st["mean"][p] - mean).max() <= REL_TOL
                assert abs(st["spreadDeg"][p] - float(ex.spreadDeg)) <= REL_TOL * max(1.0, float(ex.spreadDeg))


# ------------------------------------------------------------------------------------------------------
# 3. shards
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nsh", [("g4_n32_angles", 1), ("g4_n32_angles", 3), ("g11_n32_eulerlist", 14)])
def test_shards_merge_to_the_unsharded_sums(name, nsh):
    import bioem_amd.engine as eng
    case, S = setup_for(name)
    prior = prior_of(S)
    for algo in case["algos"]:
        E = make_engine(S, algo)
        run_native(E, S)
        whole = E.orientation_sums(prior)
        E.close()
        parts = []
        for g in range(nsh):
            o0, o1 = g * S.nAngles // nsh, (g + 1) * S.nAngles // nsh
            E = make_shard_engine(S, algo, o0, o1)
            run_shard(E, o0, o1)
            s = E.orientation_sums(prior)
            assert np.all((s["omax"] >= o0) & (s["omax"] < o1)) and np.all(s["count"] == o1 - o0)       # global indices
            parts.append(s)
            E.close()
        merged = eng.merge_orient_sums(parts)
        for f in ("m", "omax", "count", "hasMoments"):
            assert merged[f].tobytes() == whole[f].tobytes(), f
        rel = {f: np.abs(merged[f] - whole[f]) / (np.abs(whole[f]) + (whole["S0"] if f == "S1" else 0.0)) for f in SUMS}
        rel["Q"] = (np.abs(merged["Q"] - whole["Q"]) / whole["S0"][:, None]).max(axis=1)
        print("%s in %d shards, ALGO %d: max relative difference %s"
              % (name, nsh, algo, {f: "%.3g" % v.max() for f, v in rel.items()}))
        for f, v in rel.items():
            assert v.max() <= 1e-12, f


# ------------------------------------------------------------------------------------------------------
# 4. own lists on g10
# ------------------------------------------------------------------------------------------------------
def test_own_lists_on_g10_against_the_oracle():
    import bioem_amd.engine as eng
    from bioem_amd import orient_stats
    _, S = setup_for("g10_n64")
    assert S.isQuat and S.nMaps == 6 and S.nAngles == 64
    rng = np.random.default_rng(4)
    lengths = [64, 17, 0, 1, 33, 8]
    lists = [np.ascontiguousarray(S.angles[rng.permutation(S.nAngles)[:n]]) for n in lengths]
    pd = pd_of(S)
    pd.writeAngles = 5
    E = eng.Engine(pd, S.nMaps, S.nAngles, S.nCTF, algo=1, device=0)
    E.upload_particles(S.refFFT, S.sumRef, S.sumsqRef)
    E.upload_ctf(S.refCTF, S.ctfParam)
    E.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
    E.upload_particle_orientation_lists(lists, True)
    raw, pmap, pang = eng.new_prob_block(S.nMaps, S.nAngles, 5)
    E.start_run(raw)
    E.compare_own_orientations(0, S.nMaps)
    E.finish_run(raw)
    sums = E.orientation_sums(own=True)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    flat = np.concatenate([l.reshape(-1, 4) for l in lists])
    assert E.debug_orient_sums(pang, flat, True, offsets=off).tobytes() == sums.tobytes()
    with pytest.raises(RuntimeError, match="prior") as ei:
        E.orientation_sums(np.zeros(S.nAngles), own=True)
    assert ei.value.rc == 2
    E.close()
    assert list(sums["count"].astype(int)) == lengths
    st = orient_stats.derive(sums, lists)
    opd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(opd, f, getattr(S.pd, f))
    L = orc.lib()
    for p, n in enumerate(lengths):
        if n == 0:
            assert sums[p]["omax"] == -1 and sums[p]["m"] == eng.MIN_PROB and st["logZ"][p] == -np.inf
            continue
        opd.writeAngles = n
        want = np.zeros(1, dtype=orc.PROB_MAP_DTYPE)
        wang = np.zeros((n, 1), dtype=orc.PROB_ANGLE_DTYPE)
        L.orc_init_prob(1, n, n, want.ctypes.data, wang.ctypes.data)
        L.orc_run(C.byref(opd), 1, S.points.ctypes.data, len(S.points), S.NormDen, lists[p].ctypes.data, n, 1, S.px,
                  S.P["shiftX"], S.P["shiftY"], S.nCTF, S.refCTF.ctypes.data, S.ctfParam.ctypes.data, 1,
                  S.refFFT[p:p + 1].ctypes.data, S.sumRef[p:p + 1].ctypes.data, S.sumsqRef[p:p + 1].ctypes.data, 0, n,
                  want.ctypes.data, wang.ctypes.data)
        ref = R.sums(wang["forAngles"][:, 0], wang["ConstAngle"][:, 0], quats=lists[p])
        ex = R.derive(ref, lists[p][ref.omax])
        lz, H, nE = float(ex.logZ), float(ex.entropy), float(ex.nEff)
        print("particle %d (%d entries): logZ %.6f oracle %.6f | H %.6g oracle %.6g | nEff %.6g oracle %.6g | spread %.5f "
              "oracle %.5f" % (p, n, st["logZ"][p], lz, st["entropy"][p], H, st["nEff"][p], nE, st["spreadDeg"][p],
                               float(ex.spreadDeg)))
        assert int(sums[p]["omax"]) == ref.omax
        assert abs(st["logZ"][p] - lz) <= REL_TOL * abs(lz) and abs(st["logZ"][p] - lz) <= ABS_TOL
        assert abs(st["nEff"][p] - nE) <= REL_TOL * nE
        assert abs(st["entropy"][p] - H) <= REL_TOL * abs(H) + (1e-12 if n == 1 else 0.0)     # (one entry: H = 0)
        # the mean orientation: the device's and the oracle's tables differ entry by entry (float transforms; the table
        # tests allow ABS_TOL), by at most D = max - min of the differences once the common shift is taken out; the
        # weights then differ by D relative, Q / S0 by at most D in norm, and its leading eigenvector by 2 D / gap
        # (Davis-Kahan), gap = the distance of the two largest eigenvalues.  A posterior split over distant orientations
        # (particle 1: nEff 2, spread 74 degrees) has a small gap and moves more than REL_TOL for this reason alone.
        dl = (np.log(pang["forAngles"][:n, p]) + pang["ConstAngle"][:n, p]) - \
             (np.log(wang["forAngles"][:, 0]) + wang["ConstAngle"][:, 0])
        D = float(dl.max() - dl.min())
        assert D <= 2 * ABS_TOL
        w = np.linalg.eigvalsh(orient_stats.moment_matrix([float(x) for x in ref.Q]) / float(ref.S0))
        dmean = np.abs(st["mean"][p] - np.array([float(x) for x in ex.mean])).max()
        print("            mean: max difference %.3g, table difference D %.3g, gap %.3g, bound %.3g"
              % (dmean, D, w[-1] - w[-2], 2 * D / (w[-1] - w[-2])))
        assert dmean <= 2 * D / (w[-1] - w[-2]) + 1e-12
        # invariant: the log evidence over the list is the particle entry's
        assert abs(sums[p]["m"] + math.log(sums[p]["S0"]) - (math.log(pmap[p]["Total"]) + pmap[p]["Constoadd"])) <= 1e-10


# ------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    import bioem_amd.engine as eng
    _, S10 = setup_for("g10_n64")
    E = make_engine(S10, 1)                                   # a handle without WRITE_PROB_ANGLES
    assert S10.pd.writeAngles == 0
    _, before, _ = run_native(E, S10)
    out = np.zeros(S10.nMaps, dtype=eng.ORIENT_SUMS_DTYPE)
    assert E.L.bioem_hip_orientation_sums(E.h, None, 0, S10.nMaps, 0, out.ctypes.data_as(C.c_void_p)) == 2
    assert "WRITE_PROB_ANGLES" in E.L.bioem_hip_last_error(E.h).decode()
    with pytest.raises(RuntimeError, match="WRITE_PROB_ANGLES") as ei:
        E.orientation_sums()
    assert ei.value.rc == 2
    _, after, _ = run_native(E, S10)
    assert after.tobytes() == before.tobytes()
    E.close()

    _, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    _, before, _ = run_native(E, S)
    good = E.orientation_sums()
    for p0, p1 in ((-1, 2), (0, S.nMaps + 1), (2, 2), (2, 1)):
        with pytest.raises(RuntimeError, match="particle range") as ei:
            E.orientation_sums(None, p0, p1)
        assert ei.value.rc == 2
    with pytest.raises(RuntimeError, match="no per-particle orientation lists") as ei:
        E.orientation_sums(own=True)
    assert ei.value.rc == 2
    assert E.L.bioem_hip_orientation_sums(E.h, None, 0, S.nMaps, 0, None) == 2
    assert "null" in E.L.bioem_hip_last_error(E.h).decode()
    assert E.orientation_sums().tobytes() == good.tobytes()
    _, after, _ = run_native(E, S)
    assert after.tobytes() == before.tobytes()
    assert E.orientation_sums().tobytes() == good.tobytes()
    E.close()


def test_handle_fed_through_the_reference_compatible_entry():
    """bioem_hip_compare, two convolutions per call: rows staged in the entry's ring are flushed before the table is
    read; the sums are those of the kernels on the table finish_run returned, and of every orientation"""
    import bioem_amd.engine as eng
    _, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    nPar = 2
    assert S.nCTF % nPar == 0
    conv_base = np.zeros((2 * nPar, S.N, S.H, 2), dtype=np.float32)
    par_base = np.zeros(2 * nPar, dtype=eng.PARAM5_DTYPE)
    raw, pmap, pang = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
    E.start_run(raw)
    ipipe = 0
    for io in range(S.nAngles):
        conv, p5 = S.conv_spectra(io)
        for c0 in range(0, S.nCTF, nPar):
            k = (ipipe & 1) * nPar
            conv_base[k:k + nPar] = conv[c0:c0 + nPar]
            par_base[k:k + nPar] = p5[c0:c0 + nPar]
            E.compare(ipipe, io, c0, nPar, nPar, conv_base, par_base)
            ipipe += 1
    E.finish_run(raw)
    sums = E.orientation_sums()
    assert np.all(sums["count"] == S.nAngles) and sums["hasMoments"].all()
    assert E.debug_orient_sums(pang, S.angles, True).tobytes() == sums.tobytes()
    assert np.abs(sums["m"] + np.log(sums["S0"]) - (np.log(pmap["Total"]) + pmap["Constoadd"])).max() <= 1e-10
    E.close()


# ------------------------------------------------------------------------------------------------------
# 6. command line
# ------------------------------------------------------------------------------------------------------
def run_cli(args, d, env):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"
    return subprocess.run([exe] + args, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          timeout=300)


@pytest.mark.parametrize("name,shards", [("g4_n32_angles", 1), ("g4_n32_angles", 3), ("g11_n32_eulerlist", 1)])
def test_cli_orient_stats(name, shards, tmp_path):
    """the CLI's inputs are the ones this test's engine is fed, so every printed number is derive() of the engine's sums
    to the print precision: 16 significant digits, 1e-12 relative for the other grouping of the shards; the mean comes
    from the Jacobi solver instead of eigh (1e-10), and the spread goes through acos near 1, where the rounding of lambda
    is magnified to its square root (1e-5 degrees)"""
    from bioem_amd import orient_stats
    case, S = setup_for(name)
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
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientStats", "ORIENT_STATS"], d, env)
    assert r.returncode == 0, r.stdout[-2000:]
    for f in plain:
        assert open(d / f, "rb").read() == plain[f], f
    got, numconst, _ = orient_stats.parse(str(d / "ORIENT_STATS"))
    assert abs(numconst - orc.logp_constant(S.pd)) <= 1e-9 * abs(numconst)
    E = make_engine(S, 1, real_space_particles=True)
    run_native(E, S)
    want = orient_stats.derive(E.orientation_sums(prior_of(S)), S.angles)
    E.close()
    assert len(got) == S.nMaps
    for f in ("particle", "count", "omax", "hasMean"):
        assert np.array_equal(got[f], want[f]), f
    nA = 4 if S.isQuat else 3
    assert np.array_equal(got["angles"][:, :nA].astype(np.float32), S.angles[want["omax"]][:, :nA])
    tol = 1e-12
    dz = np.abs((got["logZ"] - numconst) - want["logZ"])
    print("max differences: logZ %.3g" % dz.max(), {f: "%.3g" % np.abs(got[f] - want[f]).max()
                                                   for f in ("pTop", "entropy", "nEff", "mean", "spreadDeg")})
    assert np.all(dz <= tol * np.abs(want["logZ"]) + 4e-16 * abs(numconst))
    for f in ("pTop", "entropy", "nEff"):
        assert np.all(np.abs(got[f] - want[f]) <= tol * np.maximum(np.abs(want[f]), 1.0)), f
    if S.isQuat:
        assert np.abs(got["mean"] - want["mean"]).max() <= 1e-10
        assert np.abs(got["spreadDeg"] - want["spreadDeg"]).max() <= 1e-5
    else:
        assert not got["hasMean"].any()


def test_cli_orient_stats_refusals(tmp_path):
    from bioem_amd import refine
    from test_own_lists import STEP, _write_quaternions
    env = dict(os.environ, BIOEM_ALGO="1", BIOEM_GPUS="1")
    case, _ = setup_for("g10_n64")                           # no WRITE_PROB_ANGLES in its parameter file
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, tmp_path)
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientStats", "ORIENT_STATS"], tmp_path, env)
    assert r.returncode == 1 and "--OrientStats needs WRITE_PROB_ANGLES" in r.stdout
    assert not os.path.exists(tmp_path / "ORIENT_STATS")
    case, _ = setup_for("g4_n32_angles")
    d = tmp_path / "g4"
    d.mkdir()
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    _write_quaternions(d / "grid.txt", refine.local_grid(1, STEP))
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientStats", "ORIENT_STATS", "--RefineOrientations", "grid.txt"], d, env)
    assert r.returncode == 1 and "--OrientStats is not valid with --RefineOrientations" in r.stdout
    # more shards than orientations: the run splits (orientation, CTF) pairs, an orientation's entry is spread over shards
    case, S = setup_for("g11_n32_eulerlist")
    d = tmp_path / "g11"
    d.mkdir()
    base = ["--Inputfile", os.path.join(case["dir"], "param.txt")] + write_case_inputs(case, d)
    env15 = dict(env, BIOEM_SHARDS=str(S.nAngles + 1), BIOEM_HOST_MERGE="1")
    env15.update(case["env"])
    r = run_cli(base + ["--OutputFile", "out.txt", "--OrientStats", "ORIENT_STATS"], d, env15)
    assert r.returncode == 1 and "--OrientStats is not valid with more shards than orientations" in r.stdout
    assert not os.path.exists(d / "ORIENT_STATS")
    r = run_cli(["--help"], d, env)
    assert "--OrientStats arg" in r.stdout
