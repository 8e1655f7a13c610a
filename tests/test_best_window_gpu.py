"""GPU tests of bioem_hip_window_posterior / bioem_hip_debug_window (Engine.window_posterior, best_match_window,
debug_window): the log posterior of every cell of the displacement window of a (particle, orientation, CTF) request.

Every expected value comes from tests/window_reference.py (numpy float64 and the oracle's calc_logpro), fed with spectra
the code under test did not make -- or, where the kernels alone are under test, with the very float spectra handed in.
Bounds:
  kernels alone   cc in [float(S - B) / N^2, float(S + B) / N^2], B = 8 (N^2 + 16) 2^-53 sum w |conv conj(F)|: the double
                  products, twiddles within 2 ulp, any summation order; given the device's own cc, logp within
                  16 N^2 2^-53 (|log firstele| + |log((Ntotpi - 2) ForLogProb)| + 1) of orc_calc_logpro at that cc
  whole chain     |delta logp| <= max(2e-2, 1e-4 |want|), the project's figures against the oracle (test_gpu_parity.py)
  records         norm and mu recomputed from the arg-max cell's cc to 1e-4 of the size of their terms"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle as orc
import window_reference as wr
from golden_util import load_case, oracle_setup
from test_best_maps_gpu import run_cli
from test_gpu_parity import ABS_TOL, REL_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_TOL = 1e-4


def to_engine_pd(pd):
    import bioem_amd.engine as eng
    out = eng.ParamDevice()
    for f, _ in eng.ParamDevice._fields_:
        setattr(out, f, getattr(pd, f))
    return out


def oracle_pd(base, N=None, maxD=None, grid=None):
    """a copy of the oracle's parameters with another image size / window"""
    pd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(pd, f, getattr(base, f))
    if N is not None:
        pd.NumberPixels, pd.NumberFFTPixels1D, pd.Ntotpi = N, N // 2 + 1, np.float32(N * N)
    if maxD is not None:
        pd.maxDisplaceCenter, pd.GridSpaceCenter = maxD, grid
        pd.NxDisp = 2 * (maxD // grid) + 1
        pd.NtotDisp = pd.NxDisp * pd.NxDisp
    pd.writeAngles = 0
    return pd


_setups = {}


def setup(case):
    if case not in _setups:
        _setups[case] = oracle_setup(load_case(case))
    return _setups[case]


def engine_for(S, algo=1, pd=None, maps=None, orientations=True, **kw):
    import bioem_amd.engine as eng
    maps = S.maps if maps is None else maps
    E = eng.Engine(to_engine_pd(S.pd if pd is None else pd), len(maps), S.nAngles, S.nCTF, algo=algo, device=0, **kw)
    E.upload_particle_maps(maps)
    E.upload_ctf(S.refCTF, S.ctfParam)
    E.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
    if orientations:
        E.upload_orientations(S.angles, S.isQuat)
    return E


def requests(triples):
    import bioem_amd.engine as eng
    r = np.zeros(len(triples), dtype=eng.WINDOW_REQUEST_DTYPE)
    for i, (p, o, c) in enumerate(triples):
        r[i] = (p, o, c)
    return r


def within(got, want):
    return np.abs(got - want) <= np.maximum(ABS_TOL, REL_TOL * np.abs(want))


# ---- 1. the kernels alone ----
WINDOWS = [(5, 1, 1), (5, 2, 1), (4, 2, 2)]
KERNEL_CASES = [(N, w) for N in (32, 35, 37, 64, 126, 128) for w in WINDOWS] + [(64, (20, 1, 1))]


@pytest.mark.parametrize("N,window", KERNEL_CASES)
def test_kernels_alone_to_the_derived_bounds(N, window):
    import bioem_amd.engine as eng
    maxD, grid, algo = window
    pd = oracle_pd(setup("g3_n32_trace").pd, N, maxD, grid)
    E = eng.Engine(to_engine_pd(pd), 1, 1, 1, algo=algo, device=0)
    X = E.window_shifts()
    assert X.tolist() == wr.offsets(N, maxD, grid, algo).tolist()
    nd = len(X)
    rng = np.random.default_rng(1000 * N + 10 * maxD + grid)
    # three records with different sums: a calculated image and a particle that is its shifted, scaled, noisy copy
    A = rng.standard_normal((3, N, N)) * np.array([1.0, 3.0, 0.5])[:, None, None] + np.array([0.0, 0.2, -0.1])[:, None, None]
    B = np.stack([np.roll(A[0], (2, -3), (0, 1)), 0.4 * np.roll(A[1], (-1, 0), (0, 1)), -1.5 * A[2]])
    B = B + 0.7 * rng.standard_normal((3, N, N)) + np.array([0.05, -0.3, 1.0])[:, None, None]
    conv = np.fft.rfft2(A).astype(np.complex64)
    F = np.fft.rfft2(B).astype(np.complex64)
    q = np.zeros(3, dtype=eng.PARAM5_DTYPE)
    q["amp"], q["pha"], q["env"] = 0.1, 2.0, 50.0
    q["sumC"] = conv[:, 0, 0].real
    q["sumsquareC"] = (A ** 2).sum(axis=(1, 2))
    sumRef = B.sum(axis=(1, 2)).astype(np.float32)
    sumsqRef = (B ** 2).sum(axis=(1, 2)).astype(np.float32)
    logp, cc = E.debug_window(conv, F, q, sumRef, sumsqRef)
    logp2, cc2 = E.debug_window(conv, F, q, sumRef, sumsqRef)
    E.close()
    assert logp.shape == (3, nd, nd) and cc.dtype == np.float32
    assert logp.tobytes() == logp2.tobytes() and cc.tobytes() == cc2.tobytes()
    for r in range(3):
        S, Aabs = wr.s_table(conv[r], F[r], X)
        Bnd = wr.bound(N, Aabs)
        lo, hi = wr.cc_of(S - Bnd, N), wr.cc_of(S + Bnd, N)
        print("N=%d window %s record %d: cc is the float of the reference's S in %d of %d cells, inside [lo, hi] in %d"
              % (N, window, r, int((cc[r] == wr.cc_of(S, N)).sum()), nd * nd, int(((cc[r] >= lo) & (cc[r] <= hi)).sum())))
        assert ((cc[r] >= lo) & (cc[r] <= hi)).all(), (N, window, r)
        fe = wr.firstele(pd, q[r], cc[r], sumRef[r], sumsqRef[r])
        assert (fe > 0).all() and np.isfinite(fe).all()
        want = wr.logpro(pd, q[r], cc[r], sumRef[r], sumsqRef[r])
        ratio = np.abs(logp[r] - want) / wr.logp_bound(pd, q[r], fe, N)
        print("N=%d window %s record %d: |logp - orc_calc_logpro(cc)| / bound = %.3g" % (N, window, r, ratio.max()))
        assert (ratio <= 1.0).all(), (N, window, r, np.unravel_index(int(ratio.argmax()), ratio.shape))
        if r == 0:  # the planted shift is the peak: the particle is the image rolled by (2, -3)
            i, j = np.unravel_index(int(np.argmax(logp[r])), (nd, nd))
            if 2 in X.tolist() and -3 in X.tolist():
                assert (X[i], X[j]) == (2, -3)


# ---- 2. planted shifts ----
def oracle_compare(pd, algo, maps, conv, p5, o=0, c=0):
    """orc_compare of one conv spectrum against the particle images `maps`: the oracle's records"""
    n, N = len(maps), maps.shape[1]
    ref = np.stack([orc.fft2_r2c(m) for m in maps])
    sums = np.array([orc.map_sums(m) for m in maps], dtype=np.float32)
    pmap = np.zeros(n, dtype=orc.PROB_MAP_DTYPE)
    L = orc.lib()
    L.orc_init_prob(n, 1, 0, pmap.ctypes.data_as(C.c_void_p), None)
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    sr, ssr = np.ascontiguousarray(sums[:, 0]), np.ascontiguousarray(sums[:, 1])
    cv, pp = np.ascontiguousarray(conv[None]), np.ascontiguousarray(p5.reshape(1))
    L.orc_compare(C.byref(pd), algo, n, 1, vp(ref), vp(sr), vp(ssr), o, c, 1, vp(cv), vp(pp), vp(pmap), None)
    return pmap


@pytest.mark.parametrize("case,window", [("g3_n32_trace", (5, 1, 1)), ("g9_n35_odd", (5, 2, 1))])
def test_planted_shifts_peak_where_the_oracle_reports_them(case, window):
    """the particle is the calculated image rolled by (sx, sy), sx != sy: the four corners of the set, the centre and one
    edge cell"""
    S = setup(case)
    maxD, grid, algo = window
    pd = oracle_pd(S.pd, None, maxD, grid)
    X = wr.offsets(S.N, maxD, grid, algo)
    lo, hi = int(X[0]), int(X[-1])
    o, c = S.nAngles - 1, S.nCTF // 2
    conv, p5 = S.conv_spectra(o)
    img = np.fft.irfft2(wr.as_complex(conv[c]), s=(S.N, S.N))
    corners = [(lo, lo), (lo, hi), (hi, lo), (hi, hi)]
    planted = [(0, 0), (int(X[2]), hi), (int(X[1]), 0), (lo, int(X[-2]))]  # the centre, edge cells, sx != sy
    maps = np.stack([np.roll(img, s, (0, 1)) for s in planted + corners]).astype(np.float32)
    maps += (0.01 * np.abs(img).max() * np.random.default_rng(3).standard_normal(maps.shape)).astype(np.float32)
    E = engine_for(S, algo, pd=pd, maps=maps)
    assert E.window_shifts().tolist() == X.tolist()
    t = E.window_posterior(requests([(p, o, c) for p in range(len(maps))]))
    E.close()
    want = oracle_compare(pd, algo, maps, conv[c], p5[c], o, c)
    for p in range(len(maps)):
        i, j = np.unravel_index(int(np.argmax(t[p])), t[p].shape)
        assert (X[i], X[j]) == (want[p]["cent_x"], want[p]["cent_y"]), (p, (planted + corners)[p], X[i], X[j], want[p])
        have, ref = wr.lse(t[p]), math.log(want[p]["Total"]) + want[p]["Constoadd"]
        assert within(have, ref), (p, have, ref)
    # the oracle reports what was planted, so the test means what it says
    assert [(int(w["cent_x"]), int(w["cent_y"])) for w in want] == planted + corners


# ---- 3. the chain against the oracle, every cell of every request ----
CHAIN = [("g3_n32_trace", 1, False), ("g8_n32_grid", 1, False), ("g8_n32_grid", 2, False), ("g9_n35_odd", 1, False),
         ("g13_n32_psf_writectf", 1, False), ("g10_n64", 1, False), ("g21_n64_wide20", 1, False), ("g2_n128", 1, True)]


@pytest.mark.parametrize("case,algo,part", CHAIN)
def test_chain_against_the_oracle(case, algo, part):
    S = setup(case)
    E = engine_for(S, algo)
    X = E.window_shifts()
    assert X.tolist() == wr.offsets(S.N, S.pd.maxDisplaceCenter, S.pd.GridSpaceCenter, algo).tolist()
    parts = [0, S.nMaps // 2, S.nMaps - 1] if part else list(range(S.nMaps))
    orients = [1, S.nAngles - 2] if part else list(range(S.nAngles))
    triples = [(p, o, c) for o in orients for c in range(S.nCTF) for p in parts]
    logp, cc, par = E.window_posterior(requests(triples), want_cc=True, want_params=True)
    pd = oracle_pd(S.pd)
    worst, k, skipped = 0.0, 0, 0
    for o in orients:
        conv, p5 = S.conv_spectra(o)
        for c in range(S.nCTF):
            _, sumC, sumsqC = E.debug_convolution(o, c)
            for p in parts:
                assert triples[k] == (p, o, c)
                q = par[k]
                assert (q["amp"], q["pha"], q["env"]) == tuple(S.ctfParam[c]), (k, q)
                assert q["sumC"].tobytes() == sumC.tobytes() and q["sumsquareC"].tobytes() == sumsqC.tobytes(), (k, q)
                want, _ = wr.table(pd, conv[c], S.refFFT[p], p5[c], S.sumRef[p], S.sumsqRef[p], X)
                ok = np.isfinite(want)
                skipped += int((~ok).sum())
                assert np.isfinite(logp[k][ok]).all() and within(logp[k][ok], want[ok]).all(), (case, algo, triples[k])
                worst = max(worst, float((np.abs(logp[k][ok] - want[ok]) / np.maximum(ABS_TOL, REL_TOL * np.abs(want[ok]))).max()))
                k += 1
    E.close()
    print("%s ALGO %d: %d requests x %d cells, worst |delta logp| / bound = %.3g, %d cells not finite in the reference"
          % (case, algo, len(triples), len(X) ** 2, worst, skipped))


# ---- 4. against the run ----
def device_run(E, S, o0=0, o1=None, c0=None, c1=None):
    import bioem_amd.engine as eng
    raw, pmap, _ = eng.new_prob_block(E.nMaps, S.nAngles, 0)
    E.start_run(raw)
    if c0 is None:
        E.project_convolve_compare(o0, S.nAngles if o1 is None else o1)
    else:
        E.project_convolve_compare_ctf(o0, o1, c0, c1)
    E.finish_run(raw)
    return pmap.copy()


@pytest.mark.parametrize("case", ["g3_n32_trace", "g10_n64", "g9_n35_odd"])
def test_best_match_window_against_the_run(case):
    S = setup(case)
    E = engine_for(S, 1)
    pmap = device_run(E, S)
    t, cc = E.best_match_window(pmap, want_cc=True)
    X = E.window_shifts()
    _, sumRef, _ = E.debug_particles()
    f = np.float32
    Np = f(S.pd.Ntotpi)
    for p in range(S.nMaps):
        r = pmap[p]
        o, c = int(r["orient"]), int(r["conv"])
        i, j = np.unravel_index(int(np.argmax(t[p])), t[p].shape)
        assert (X[i], X[j]) == (r["cent_x"], r["cent_y"]), (p, X[i], X[j], r)
        one = device_run(E, S, o, o + 1, c, c + 1)[p]
        assert (one["orient"], one["conv"]) == (o, c)
        have, want = wr.lse(t[p]), math.log(one["Total"]) + one["Constoadd"]
        assert within(have, want), (p, have, want)
        # norm and mu of the record from the arg-max cell's cc (bioem_algorithm.h:101-104), in float
        _, sumC, sumsqC = E.debug_convolution(o, c)
        v, sr = f(cc[p, i, j]), f(sumRef[p])
        den = f(f(sumC * sumC) - f(sumsqC * Np))
        norm = -f(f(f(-sumC) * sr) + f(Np * v)) / den
        mu = -f(f(f(-sumC) * v) + f(sumsqC * sr)) / den
        sn = (abs(float(sumC) * float(sr)) + abs(float(Np) * float(v))) / abs(float(den))
        sm = (abs(float(sumC) * float(v)) + abs(float(sumsqC) * float(sr))) / abs(float(den))
        assert abs(float(norm) - float(r["norm"])) <= CHAIN_TOL * sn, (p, norm, r["norm"])
        assert abs(float(mu) - float(r["mu"])) <= CHAIN_TOL * sm, (p, mu, r["mu"])
    E.close()


# ---- 5. batches and order ----
def test_batches_and_order_bit_identical():
    """2 maxOrientations + 3 requests with repeated and permuted particles: the same bits as one-request calls, in a
    repeated call and in the reversed list"""
    S = setup("g8_n32_grid")
    E = engine_for(S, 1)
    maxO = E.max_batch()[0]
    n = 2 * maxO + 3
    distinct = [(p, o, c) for p in range(S.nMaps) for o in range(S.nAngles) for c in range(S.nCTF)]
    order = np.random.default_rng(17).permutation(len(distinct))
    triples = [distinct[order[(5 * i) % len(distinct)]] for i in range(n)]
    triples[1] = triples[0]                    # a repeat side by side
    triples[maxO] = triples[maxO - 1]          # and one across the batch boundary
    req = requests(triples)
    full, ccs, par = E.window_posterior(req, want_cc=True, want_params=True)
    again = E.window_posterior(req)
    assert full.tobytes() == again.tobytes()
    back, ccb, parb = E.window_posterior(req[::-1].copy(), want_cc=True, want_params=True)
    assert back[::-1].tobytes() == full.tobytes() and ccb[::-1].tobytes() == ccs.tobytes()
    assert parb[::-1].tobytes() == par.tobytes()
    single = {}
    for k, tr in enumerate(triples):
        if tr not in single:
            single[tr] = E.window_posterior(requests([tr]), want_cc=True, want_params=True)
        one, occ, opar = single[tr]
        assert one[0].tobytes() == full[k].tobytes(), (k, tr)
        assert occ[0].tobytes() == ccs[k].tobytes() and opar[0].tobytes() == par[k].tobytes(), (k, tr)
    E.close()
    assert n > 2 * maxO and len(single) >= 4


# ---- 6. own lists ----
def test_own_lists_bit_identical_to_the_shared_list():
    S = setup("g8_n32_grid")
    E = engine_for(S, 1)
    with pytest.raises(RuntimeError, match="lists") as e:
        E.window_posterior(requests([(0, 0, 0)]), own=True)
    assert e.value.rc == 2
    perm = [np.random.default_rng(40 + p).permutation(S.nAngles)[:S.nAngles - 2 * p] for p in range(S.nMaps)]
    E.upload_particle_orientation_lists([S.angles[q] for q in perm], S.isQuat)
    own, shared = [], []
    for p in range(S.nMaps):
        for k in (0, len(perm[p]) - 1, len(perm[p]) // 2):
            for c in (0, S.nCTF - 1):
                own.append((p, k, c))
                shared.append((p, int(perm[p][k]), c))
    a = E.window_posterior(requests(own), own=True, want_cc=True, want_params=True)
    b = E.window_posterior(requests(shared), want_cc=True, want_params=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    with pytest.raises(RuntimeError, match="request 1") as e:  # beyond particle 1's shorter list
        E.window_posterior(requests([(0, 0, 0), (1, len(perm[1]), 0)]), own=True)
    assert e.value.rc == 2
    E.close()


# ---- 7. refusals, handle kinds ----
def test_refusals_name_the_request_and_leave_the_handle_usable():
    import bioem_amd.engine as eng
    S = setup("g3_n32_trace")
    E = engine_for(S, 1)
    good = requests([(0, 0, 0), (1, S.nAngles - 1, S.nCTF - 1), (0, 1, 1)])
    ref = E.window_posterior(good).tobytes()

    def refused(req, **kw):
        with pytest.raises(RuntimeError) as e:
            E.window_posterior(req, **kw)
        assert e.value.rc == 2, str(e.value)
        assert E.window_posterior(good).tobytes() == ref
        return str(e.value)

    for field, value in (("particle", S.nMaps), ("particle", -1), ("orient", S.nAngles), ("orient", -1),
                         ("conv", S.nCTF), ("conv", -1)):
        bad = good.copy()
        bad[2][field] = value
        assert "request 2" in refused(bad), (field, value)
    refused(good[:0])
    refused(good, own=True)
    assert E.L.bioem_hip_window_posterior(E.h, None, 1, 0, None, None, None) == 2
    out = np.zeros(1)
    assert E.L.bioem_hip_debug_window(E.h, None, None, None, None, None, 1, out.ctypes.data_as(C.c_void_p), None) == 2
    assert E.window_posterior(good).tobytes() == ref
    E.close()
    # nothing uploaded: model, CTFs, orientations, particles
    E2 = eng.Engine(to_engine_pd(S.pd), S.nMaps, S.nAngles, S.nCTF, algo=1, device=0)
    for step in (lambda: E2.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"]),
                 lambda: E2.upload_ctf(S.refCTF, S.ctfParam),
                 lambda: E2.upload_orientations(S.angles, S.isQuat),
                 lambda: E2.upload_particle_maps(S.maps)):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.window_posterior(good)
        assert e.value.rc == 2
        step()
    assert E2.window_posterior(good).tobytes() == ref
    E2.close()


def test_shard_and_algo2_handles():
    """a shard handle (which is what a CTF-split run creates, too: the plain handle) serves global requests with the
    plain handle's bytes; an ALGO 2 handle returns its own set of cells"""
    S = setup("g8_n32_grid")
    req = requests([(p, o, c) for p in range(S.nMaps) for o in (0, S.nAngles - 1) for c in (0, S.nCTF - 1)])
    E = engine_for(S, 1)
    ref = E.window_posterior(req)
    E.set_phase_timing(True)
    E.window_posterior(req)
    ph = E.phase_records()
    E.set_phase_timing(False)
    nB = -(-len(req) // E.max_batch()[0])
    assert sorted(ph["phase"].tolist()) == [0] * nB + [1] * nB + [2] * nB and (ph["seconds"] > 0).all()
    E.close()
    Es = engine_for(S, 1, shard=(2, 5))
    assert Es.window_posterior(req).tobytes() == ref.tobytes()
    Es.close()
    E2 = engine_for(S, 2)
    X1 = wr.offsets(S.N, S.pd.maxDisplaceCenter, S.pd.GridSpaceCenter, 1)
    X2 = E2.window_shifts()
    assert X2.tolist() == wr.offsets(S.N, S.pd.maxDisplaceCenter, S.pd.GridSpaceCenter, 2).tolist() != X1.tolist()
    t2 = E2.window_posterior(req)
    E2.close()
    assert t2.shape[1:] == (len(X2), len(X2))
    both = [x for x in X2.tolist() if x in X1.tolist()]
    i1, i2 = [X1.tolist().index(x) for x in both], [X2.tolist().index(x) for x in both]
    assert len(both) >= 2 and t2[:, i2][:, :, i2].tobytes() == ref[:, i1][:, :, i1].tobytes()  # a cell is a cell


# ---- 8. CLI ----
def test_cli_best_window(tmp_path):
    """--BestWindow on a golden case: the parsed file equals derive() of best_match_window on the run's records;
    Output_Probabilities is byte-identical to the run without the option; with --RefineOrientations FILE and FILE_Round2"""
    import bioem_amd.engine as eng
    from bioem_amd import best_window as bw, hostlib, refine
    from golden_util import write_case_inputs
    case = load_case("g10_n64")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--BestWindow", "win.txt"], d, BIOEM_ALGO="1")
    assert "win.txt" in out
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    S, angles, ref, par = hostlib.setup_from_files(param, str(d / "orient.txt") if case["orient_lines"] else None)
    pts, nden = hostlib.read_model(str(d / "model.txt"), nocentermass=bool(S.nocentermass), pixelSize=S.pixelSize)
    maps = hostlib.read_particles(str(d / "particles.txt"), S.pd.NumberPixels)
    E = eng.Engine(S.pd, len(maps), S.nAngles, S.nCTF, algo=1, device=0)
    E.upload_particle_maps(maps)
    E.upload_ctf(ref, par)
    E.upload_model(pts, nden, S.pixelSize, S.shiftX, S.shiftY)
    E.upload_orientations(angles, S.isQuat)
    raw, pmap, _ = eng.new_prob_block(len(maps), S.nAngles, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    t = E.best_match_window(pmap)
    X = E.window_shifts()
    E.close()
    numconst = orc.logp_constant(S.pd)
    want, W = bw.derive(t + numconst, X)
    summ, cells, _ = bw.parse(str(d / "win.txt"))
    assert len(summ) == len(maps)
    for p in range(len(maps)):
        assert summ[p]["orient"] == pmap[p]["orient"] and summ[p]["nd"] == len(X)
        assert (summ[p]["peakX"], summ[p]["peakY"]) == (pmap[p]["cent_x"], pmap[p]["cent_y"])
        for f in bw.STAT_FIELDS:
            a, b = float(summ[p][f]), float(want[p][f])
            assert a == b or abs(a - b) <= 1e-12 * max(abs(b), 1e-3), (p, f, a, b)
        assert (np.abs(cells[p]["logp"] - (t[p] + numconst)) <= 1e-12 * np.abs(t[p] + numconst)).all()
        assert (np.abs(cells[p]["weight"] - W[p]) <= 1e-12).all()
        assert (cells[p]["X"] == X[:, None]).all() and (cells[p]["Y"] == X[None, :]).all()
        lp = math.log(pmap[p]["Total"]) + pmap[p]["Constoadd"] + numconst
        assert summ[p]["logP"] <= lp + max(ABS_TOL, REL_TOL * abs(lp))  # one pair's share of the particle's evidence
    if S.isQuat:
        q = refine.local_grid(1, 0.05)
        with open(d / "grid.txt", "w") as f:
            f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
        run_cli(inputs + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--BestWindow", "winr.txt"], d,
                BIOEM_ALGO="1")
        assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
        assert open(d / "winr.txt", "rb").read() == open(d / "win.txt", "rb").read()
        s2, c2, _ = bw.parse(str(d / "winr.txt_Round2"))
        assert len(s2) == len(maps) and (s2["nd"] == len(X)).all() and np.isfinite(s2["logP"]).all()
