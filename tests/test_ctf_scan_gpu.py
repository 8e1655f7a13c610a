"""GPU tests of bioem_hip_ctf_scan / bioem_hip_debug_ctf_scan (Engine.ctf_scan, best_match_ctf_scan, debug_ctf_scan): the
log posterior of a (particle, orientation, shift) record under every CTF set of a list handed in.

Every expected value comes from tests/window_reference.py (numpy float64 and the oracle's calc_logpro), the oracle and
numpy, fed with spectra the code under test did not make -- or, where the scan kernels alone are under test, with the very
float spectra handed in.  Bounds:
  sumC, sumsquareC  bit for bit: the float product written out unfused, the Parseval terms added one after the other in
                    float32 in the reference's order (rows; the interior columns doubled, column 0, column N / 2), / N^2
  cc                in [float(S - B) / N^2, float(S + B) / N^2], S the reference's sum at the request's cell and
                    B = window_reference.bound(N, A) (the scan's N H terms fit under the window pass's bound)
  logp              given the device's own cc, within window_reference.logp_bound of orc_calc_logpro at that cc
  whole chain       |delta logp| <= max(2e-2, 1e-4 |want|), the project's figures against the oracle (test_gpu_parity.py)"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
import window_reference as wr
from golden_util import load_case, oracle_setup, write_case_inputs
from test_best_maps_gpu import run_cli
from test_best_window_gpu import device_run, engine_for, oracle_pd, setup, to_engine_pd, within
from test_gpu_parity import ABS_TOL, REL_TOL

pytestmark = pytest.mark.gpu


def scan_requests(rows):
    import bioem_amd.engine as eng
    r = np.zeros(len(rows), dtype=eng.SCAN_REQUEST_DTYPE)
    for i, row in enumerate(rows):
        r[i] = tuple(int(v) for v in row)
    return r


def walk_order(N):
    """(flat indices e = kx H + ky of an [N, H] spectrum in the order of the reference's Parseval sum, True where the term
    is doubled): bioem.cpp:1896-1914"""
    H = N // 2 + 1
    jend = H if N % 2 else H - 1
    cols = list(range(1, jend)) + [0] + ([H - 1] if N % 2 == 0 else [])
    dbl = [True] * (jend - 1) + [False] + ([False] if N % 2 == 0 else [])
    order = np.array([i * H + j for i in range(N) for j in cols])
    assert sorted(order.tolist()) == list(range(N * H))
    return order, np.array(dbl * N)


def definition(P, kernels):
    """conv [G, N, H, 2], sumC [G], sumsquareC [G] of one projection spectrum P [N, H, 2] against the kernels [G, N, H, 2]:
    float32 throughout, every operation rounded on its own"""
    P, K = np.asarray(P, dtype=np.float32), np.asarray(kernels, dtype=np.float32)
    N = P.shape[0]
    ox = P[None, ..., 0] * K[..., 0] + P[None, ..., 1] * K[..., 1]
    oy = P[None, ..., 1] * K[..., 0] - P[None, ..., 0] * K[..., 1]
    assert ox.dtype == np.float32
    t = (ox * ox + oy * oy).reshape(len(K), -1)
    order, dbl = walk_order(N)
    tw = t[:, order]
    tw[:, dbl] = tw[:, dbl] * np.float32(2)
    ss = np.cumsum(tw, axis=1, dtype=np.float32)[:, -1] / np.float32(N * N)  # a strict chain: cumsum adds one by one
    return np.stack([ox, oy], axis=-1), ox[:, 0, 0].copy(), ss


def s_at(conv, F, X, Y):
    """the reference's S at the reported shift (X, Y) and A = sum w |conv conj(F)|"""
    S, A = wr.s_map(conv, F)
    N = S.shape[0]
    return S[(-int(X)) % N, (-int(Y)) % N], A


def check_against_the_definition(pd, N, P, F, kernels, par3, shifts, sumRef, sumsqRef, cc, logp, par, what):
    """cc [n, G], logp [n, G], par [n, G] of the device against the definition for records (P[r], F[r], shifts[r]);
    returns the largest |logp - orc_calc_logpro(cc)| / bound"""
    worst = 0.0
    for r in range(len(P)):
        conv, sumC, ss = definition(P[r], kernels)
        assert par["sumC"][r].tobytes() == sumC.tobytes(), (what, r)
        assert par["sumsquareC"][r].tobytes() == ss.tobytes(), (what, r, np.flatnonzero(par["sumsquareC"][r] != ss)[:5])
        assert par["amp"][r].tobytes() == par3[:, 0].tobytes() and par["pha"][r].tobytes() == par3[:, 1].tobytes()
        assert par["env"][r].tobytes() == par3[:, 2].tobytes()
        for g in range(len(kernels)):
            S, A = s_at(conv[g], F[r], shifts[r][0], shifts[r][1])
            B = wr.bound(N, A)
            lo, hi = wr.cc_of(S - B, N), wr.cc_of(S + B, N)
            assert lo <= cc[r, g] <= hi, (what, r, g, lo, cc[r, g], hi)
            q = par[r, g]
            fe = wr.firstele(pd, q, cc[r, g], sumRef[r], sumsqRef[r])
            assert fe > 0 and np.isfinite(fe), (what, r, g, fe)
            want = wr.logpro(pd, q, cc[r, g], sumRef[r], sumsqRef[r])
            ratio = float(abs(logp[r, g] - want) / wr.logp_bound(pd, q, fe, N))
            assert ratio <= 1.0, (what, r, g, logp[r, g], want)
            worst = max(worst, ratio)
    return worst


# ---- 1. the kernels alone ----
NMAX, GMAX = 9, 130
_alone = {}


def alone_data(N):
    """9 records and 130 candidates at image size N, made once: calculated images, particles that are their shifted,
    scaled, noisy copies, kernels that are the spectra of random real images near a delta, and the shifts (0, 0), the two
    extreme ones and interior ones"""
    if N not in _alone:
        rng = np.random.default_rng(7000 + N)
        scale = rng.uniform(0.5, 3.0, NMAX)[:, None, None]
        A = rng.standard_normal((NMAX, N, N)) * scale + rng.uniform(-0.2, 0.2, NMAX)[:, None, None]
        base = [(0, 0), (N - 1, -(N - 1)), (-(N - 1), N - 1), (3, -2)]
        shifts = np.array([base[r % 4] if r < 8 else (-5, N // 2) for r in range(NMAX)], dtype=np.int32)
        kimg = 0.3 * rng.standard_normal((GMAX, N, N)) / N
        kimg[:, 0, 0] += 1.0
        kernels = np.fft.rfft2(kimg).astype(np.complex64)
        Kf = np.ascontiguousarray(kernels).view(np.float32).reshape(GMAX, N, N // 2 + 1, 2)
        # the particle of record r: its image under candidate r, rolled to its shift, scaled, offset, with noise
        conv_img = np.fft.irfft2(np.fft.rfft2(A) * np.conj(kernels[:NMAX].astype(np.complex128)), s=(N, N))
        B = np.stack([np.roll(conv_img[r], tuple(shifts[r]), (0, 1)) for r in range(NMAX)])
        B = rng.uniform(0.4, 1.5, NMAX)[:, None, None] * B + 0.7 * scale * rng.standard_normal((NMAX, N, N))
        B = (B + rng.uniform(-0.3, 1.0, NMAX)[:, None, None]).astype(np.float32)
        P = np.ascontiguousarray(np.fft.rfft2(A).astype(np.complex64)).view(np.float32).reshape(NMAX, N, N // 2 + 1, 2)
        F = np.ascontiguousarray(np.fft.rfft2(B).astype(np.complex64)).view(np.float32).reshape(NMAX, N, N // 2 + 1, 2)
        par3 = np.stack([rng.uniform(0.05, 0.5, GMAX), rng.uniform(1000.0, 3000.0, GMAX), rng.uniform(20.0, 200.0, GMAX)],
                        axis=1).astype(np.float32)
        sumRef = B.astype(np.float64).sum(axis=(1, 2)).astype(np.float32)
        sumsqRef = (B.astype(np.float64) ** 2).sum(axis=(1, 2)).astype(np.float32)
        _alone[N] = dict(P=P, F=F, K=Kf, par3=par3, shifts=shifts, sumRef=sumRef, sumsqRef=sumsqRef)
    return _alone[N]


def alone_engine(N, nAngles=16):
    """a handle with parameters only; its batch holds nAngles records"""
    import bioem_amd.engine as eng
    pd = oracle_pd(setup("g3_n32_trace").pd, N, 5, 1)
    return eng.Engine(to_engine_pd(pd), 1, nAngles, 1, algo=1, device=0), pd


def alone_run(E, D, n, G, rec=None, cand=None):
    rec = np.arange(n) if rec is None else np.asarray(rec)
    cand = np.arange(G) if cand is None else np.asarray(cand)
    return E.debug_ctf_scan(D["P"][rec], D["F"][rec], D["sumRef"][rec], D["sumsqRef"][rec], D["shifts"][rec], D["K"][cand],
                            D["par3"][cand])


SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (9, 130)]


@pytest.mark.parametrize("N", [32, 35, 37, 64])
def test_kernels_alone_to_the_derived_bounds(N):
    """record counts at the edges of the groups a wave may carry (1, 2 or 4 records, a compile-time choice), candidate
    counts at the edges of the 64-lane chunks"""
    D = alone_data(N)
    E, pd = alone_engine(N)
    assert E.max_batch()[0] >= NMAX  # the nine records share a batch: groups of records are what is under test
    for n, G in SHAPES + ([(9, 1), (1, 130)] if N == 35 else []):
        logp, cc, par = alone_run(E, D, n, G)
        assert logp.shape == (n, G) and cc.dtype == np.float32 and logp.dtype == np.float64
        worst = check_against_the_definition(pd, N, D["P"][:n], D["F"][:n], D["K"][:G], D["par3"][:G], D["shifts"][:n],
                                             D["sumRef"][:n], D["sumsqRef"][:n], cc, logp, par, (N, n, G))
        print("N=%d n=%d G=%d: sumC and sumsquareC bit for bit, cc inside [lo, hi], |logp - orc_calc_logpro(cc)| / bound "
              "<= %.3g" % (N, n, G, worst))
        if n == NMAX and G == GMAX:  # (record r's particle was made with candidate r at its shift)
            print("N=%d: arg-max candidate per record %s" % (N, np.argmax(logp, axis=1).tolist()))
    E.close()


# ---- 2. the same bits in any order, subset, split and batch ----
def test_same_bits_for_any_order_subset_split_and_batch():
    N = 35
    D = alone_data(N)
    E, _ = alone_engine(N)
    full = alone_run(E, D, NMAX, GMAX)
    again = alone_run(E, D, NMAX, GMAX)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()

    def same(got, rec, cand, what):
        for a, b in zip(got, full):
            assert a.tobytes() == np.ascontiguousarray(b[np.ix_(rec, cand)]).tobytes(), what

    rng = np.random.default_rng(3)
    allr, allc = np.arange(NMAX), np.arange(GMAX)
    pc, pr = rng.permutation(GMAX), rng.permutation(NMAX)
    same(alone_run(E, D, 0, 0, allr, pc), allr, pc, "candidates permuted")
    same(alone_run(E, D, 0, 0, pr, allc), pr, allc, "requests permuted")
    same(alone_run(E, D, 0, 0, pr, pc), pr, pc, "both permuted")
    sc, sr = np.array([129, 3, 64, 63, 65, 3, 0]), np.array([8, 2, 2, 5, 0])
    same(alone_run(E, D, 0, 0, allr, sc), allr, sc, "a subset of the candidates, one twice")
    same(alone_run(E, D, 0, 0, sr, allc), sr, allc, "a subset of the requests, one twice")
    same(alone_run(E, D, 0, 0, sr, sc), sr, sc, "subsets of both")
    for cut in (1, 64, 70):
        for part in (allc[:cut], allc[cut:]):
            same(alone_run(E, D, 0, 0, allr, part), allr, part, ("G split over two calls", cut))
    E.close()
    for nAngles in (1, 2, 5):  # the batch edge moves: 9 records in batches of 1, 2, 5
        E2, _ = alone_engine(N, nAngles)
        assert E2.max_batch()[0] == nAngles
        same(alone_run(E2, D, NMAX, GMAX), allr, allc, ("maxOrientations", nAngles))
        if nAngles == 1:  # 20 records in batches of one: more than one launch of the scan serves (16 batches)
            many = np.arange(20) % NMAX
            same(alone_run(E2, D, 0, 0, many, sc), many, sc, "two launches")
        E2.close()


# ---- 3. against the window posterior ----
@pytest.mark.parametrize("case", ["g8_n32_grid", "g10_n64", "g13_n32_psf_writectf"])
def test_own_sets_at_window_cells_against_the_window_posterior(case):
    """the handle's own CTF sets as candidates, requests over the corners and the centre of the window: the parameters are
    those of window_posterior bit for bit; cc and logp are held against the definition evaluated on the projection and
    particle spectra the handle holds (no equality of the two entries' cc: their sums run in different orders)"""
    import bioem_amd.engine as eng
    S = setup(case)
    E = engine_for(S, 1)
    X = E.window_shifts()
    cells = [(X[0], X[0]), (X[0], X[-1]), (X[-1], X[0]), (X[-1], X[-1]), (X[len(X) // 2], X[len(X) // 2])]
    pairs = [(0, 1), (S.nMaps - 1, S.nAngles - 1), (S.nMaps // 2, S.nAngles // 2)]
    rows = [(p, o, x, y) for (p, o) in pairs for (x, y) in cells]
    logp, cc, par = E.ctf_scan(scan_requests(rows), S.refCTF, S.ctfParam, want_cc=True, want_params=True)
    assert logp.shape == (len(rows), S.nCTF)
    wreq = np.zeros(len(pairs) * S.nCTF, dtype=eng.WINDOW_REQUEST_DTYPE)
    for k, (p, o) in enumerate(pairs):
        for c in range(S.nCTF):
            wreq[k * S.nCTF + c] = (p, o, c)
    wlogp, wcc, wpar = E.window_posterior(wreq, want_cc=True, want_params=True)
    spec, sumRef, sumsqRef = E.debug_particles()
    pd = oracle_pd(S.pd)
    ix = {int(x): i for i, x in enumerate(X)}
    nearest = 0
    for k, (p, o) in enumerate(pairs):
        for c in range(S.nCTF):
            _, sumC, sumsqC = E.debug_convolution(o, c)
            for j in range(len(cells)):
                q = par[k * len(cells) + j, c]
                assert q.tobytes() == wpar[k * S.nCTF + c].tobytes(), (case, p, o, c)
                assert q["sumC"].tobytes() == sumC.tobytes() and q["sumsquareC"].tobytes() == sumsqC.tobytes()
        P = E.debug_projection(o)
        sl = slice(k * len(cells), (k + 1) * len(cells))
        n = len(cells)
        check_against_the_definition(pd, S.N, np.repeat(P[None], n, 0), np.repeat(spec[p][None], n, 0), S.refCTF, S.ctfParam,
                                     cells, np.repeat(sumRef[p], n), np.repeat(sumsqRef[p], n), cc[sl], logp[sl], par[sl],
                                     (case, p, o))
        for j, (x, y) in enumerate(cells):  # (the two entries' sums run in different orders: counted, not asserted)
            for c in range(S.nCTF):
                nearest += int(cc[k * n + j, c] != wcc[k * S.nCTF + c, ix[int(x)], ix[int(y)]])
    print("%s: %d (request, set) pairs, cc not the float of the window entry's in %d" % (case, logp.size, nearest))
    E.close()


# ---- 4. the whole chain against the oracle, off the grid ----
def doubled_setup(case):
    """the oracle's set-up with the CTF grid counts doubled on every axis that has more than one point: the same range, a
    step half as wide, so every other candidate is a set of the run and the others are not"""
    c = load_case(case)
    P = dict(c["P"])
    for k in ("nAmp", "nPhase", "nEnv"):
        if P[k] > 1:
            P[k] = 2 * P[k]
    return orc.Setup(P, c["model"], c["maps"], c["orient_lines"])


def oracle_scan(S, cand, p, o, x, y, X):
    """wr.table at the cell (x, y) of particle p, orientation o under every candidate of the set-up cand"""
    proj = orc.projection(S.points, S.NormDen, S.angles[o], S.isQuat, S.N, S.px, S.P["shiftX"], S.P["shiftY"])
    pd = oracle_pd(S.pd)
    i, j = X.tolist().index(x), X.tolist().index(y)
    out = np.zeros(cand.nCTF)
    for g in range(cand.nCTF):
        conv, sC, ssC = orc.convolve(proj, cand.refCTF[g])
        q = dict(amp=cand.ctfParam[g, 0], pha=cand.ctfParam[g, 1], env=cand.ctfParam[g, 2], sumC=sC, sumsquareC=ssC)
        t, _ = wr.table(pd, conv, S.refFFT[p], q, S.sumRef[p], S.sumsqRef[p], X)
        out[g] = t[i, j]
    return out


@pytest.mark.parametrize("case", ["g8_n32_grid", "g9_n35_odd", "g10_n64"])
def test_chain_against_the_oracle_off_the_grid(case):
    S = setup(case)
    cand = doubled_setup(case)
    assert cand.nCTF > S.nCTF and cand.nCTF <= 64
    on_grid = sum(any((cand.ctfParam[g] == S.ctfParam[c]).all() for c in range(S.nCTF)) for g in range(cand.nCTF))
    assert on_grid == S.nCTF  # the run's sets are among the candidates, the others lie between them
    E = engine_for(S, 1)
    X = E.window_shifts()
    rows = [(0, 0, X[0], X[-1]), (S.nMaps - 1, S.nAngles - 1, X[len(X) // 2], X[1]), (S.nMaps // 2, S.nAngles // 2, X[-1], X[0]),
            (0, S.nAngles - 2, X[2], X[2])]
    logp = E.ctf_scan(scan_requests(rows), cand.refCTF, cand.ctfParam)
    E.close()
    worst = 0.0
    for k, (p, o, x, y) in enumerate(rows):
        want = oracle_scan(S, cand, p, o, int(x), int(y), X)
        ok = np.isfinite(want)
        assert ok.sum() >= cand.nCTF // 2
        assert np.isfinite(logp[k][ok]).all() and within(logp[k][ok], want[ok]).all(), (case, rows[k], logp[k], want)
        worst = max(worst, float((np.abs(logp[k][ok] - want[ok]) / np.maximum(ABS_TOL, REL_TOL * np.abs(want[ok]))).max()))
    print("%s: %d requests x %d candidates, worst |delta logp| / bound = %.3g" % (case, len(rows), cand.nCTF, worst))


# ---- 5. planted truth ----
def test_planted_candidate_between_two_grid_sets_is_found():
    """one particle rendered by the oracle, without noise, with a candidate halfway between two defocus values of the grid
    at a shift inside the window: after a run on the coarse grid the scan at k = 4 peaks on the planted candidate; the
    run's own best set is one of its two grid neighbours"""
    import bioem_amd.engine as eng
    from bioem_amd import ctf_scan as cs, hostlib
    case = load_case("g8_n32_grid")
    S0 = setup("g8_n32_grid")
    P = case["P"]
    k = 4
    triples, counts = cs.refine_grid(P, k)
    assert counts.tolist() == [1, 2 * k, 2 * k] and not P["usepsf"]
    kernels = hostlib.ctf_kernel_list(S0.N, S0.px, triples)
    ip, ie = k // 2, k  # halfway between the defocus values 0 and 1 of the grid, at its envelope value 1
    g = ip * counts[2] + ie
    neighbours = [0 * P["nEnv"] + 1, 1 * P["nEnv"] + 1]
    assert (triples[0 * counts[2] + ie] == S0.ctfParam[neighbours[0]]).all()
    assert (triples[k * counts[2] + ie] == S0.ctfParam[neighbours[1]]).all()
    assert S0.ctfParam[neighbours[0], 1] < triples[g, 1] < S0.ctfParam[neighbours[1], 1]
    o = 3
    X = wr.offsets(S0.N, S0.pd.maxDisplaceCenter, S0.pd.GridSpaceCenter, 1)
    sx, sy = int(X[1]), int(X[-2])
    proj = orc.projection(S0.points, S0.NormDen, S0.angles[o], S0.isQuat, S0.N, S0.px, P["shiftX"], P["shiftY"])
    conv, _, _ = orc.convolve(proj, kernels[g])
    img = np.fft.irfft2(wr.as_complex(conv), s=(S0.N, S0.N)) / (S0.N * S0.N)
    part = (2.5 * np.roll(img, (sx, sy), (0, 1)) + 0.3).astype(np.float32)
    S = orc.Setup(P, case["model"], part[None], case["orient_lines"])
    E = engine_for(S, 1)
    pmap = device_run(E, S)
    rec = pmap[0]
    assert (rec["orient"], rec["cent_x"], rec["cent_y"]) == (o, sx, sy), rec
    assert int(rec["conv"]) in neighbours, rec
    logp = E.best_match_ctf_scan(pmap, kernels, triples)
    E.close()
    summ, w, marg = cs.derive(logp, triples, counts)
    print("planted candidate %d %s: arg-max %d, n_eff %.3g, mean defocus axis %.6g" % (g, triples[g], summ[0]["best"],
                                                                                         summ[0]["n_eff"], summ[0]["mean"][1]))
    assert logp.shape == (1, len(triples)) and int(np.nanargmax(logp[0])) == g and summ[0]["best"] == g


# ---- 6. refusals, handle kinds ----
def test_refusals_name_the_offender_and_leave_the_handle_usable():
    import bioem_amd.engine as eng
    S = setup("g8_n32_grid")
    N = S.N
    E = engine_for(S, 1)
    good = scan_requests([(0, 0, 0, 0), (1, S.nAngles - 1, N - 1, -(N - 1)), (0, 1, -3, 2)])
    ref = [a.tobytes() for a in E.ctf_scan(good, S.refCTF, S.ctfParam, want_cc=True, want_params=True)]
    D = alone_data(32)
    assert N == 32
    small = [a.tobytes() for a in alone_run(E, D, 1, 1)]

    def usable(Eh):
        assert [a.tobytes() for a in Eh.ctf_scan(good, S.refCTF, S.ctfParam, want_cc=True, want_params=True)] == ref
        assert [a.tobytes() for a in alone_run(Eh, D, 1, 1)] == small

    def refused(req, kernels=S.refCTF, par3=S.ctfParam, **kw):
        with pytest.raises(RuntimeError) as e:
            E.ctf_scan(req, kernels, par3, **kw)
        assert e.value.rc == 2, str(e.value)
        usable(E)
        return str(e.value)

    for field, value in (("particle", S.nMaps), ("particle", -1), ("orient", S.nAngles), ("orient", -1), ("shiftX", N),
                         ("shiftX", -N), ("shiftY", N), ("shiftY", -N)):
        bad = good.copy()
        bad[2][field] = value
        msg = refused(bad)
        assert "request 2" in msg and field[:5] in msg, (field, value, msg)
    refused(good[:0])
    assert "G = 0" in refused(good, S.refCTF[:0], S.ctfParam[:0])
    assert "lists" in refused(good, own=True)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros((3, S.nCTF))
    k, t = np.ascontiguousarray(S.refCTF), np.ascontiguousarray(S.ctfParam)
    L = E.L
    assert L.bioem_hip_ctf_scan(E.h, vp(good), 3, 0, None, vp(t), S.nCTF, vp(out), None, None) == 2
    assert b"kernels" in L.bioem_hip_last_error(E.h)
    assert L.bioem_hip_ctf_scan(E.h, vp(good), 3, 0, vp(k), None, S.nCTF, vp(out), None, None) == 2
    assert L.bioem_hip_ctf_scan(E.h, vp(good), 3, 0, vp(k), vp(t), S.nCTF, None, None, None) == 2
    assert L.bioem_hip_ctf_scan(E.h, None, 3, 0, vp(k), vp(t), S.nCTF, vp(out), None, None) == 2
    assert L.bioem_hip_ctf_scan(E.h, vp(good), 3, 0, vp(k), vp(t), -1, vp(out), None, None) == 2
    sh = np.array([[0, N]], dtype=np.int32)
    with pytest.raises(RuntimeError, match="record 0") as e:
        E.debug_ctf_scan(D["P"][:1], D["F"][:1], D["sumRef"][:1], D["sumsqRef"][:1], sh, D["K"][:1], D["par3"][:1])
    assert e.value.rc == 2
    with pytest.raises(RuntimeError) as e:
        E.debug_ctf_scan(D["P"][:1], D["F"][:1], D["sumRef"][:1], D["sumsqRef"][:1], sh * 0, D["K"][:0], D["par3"][:0])
    assert e.value.rc == 2
    usable(E)
    # an own-list index beyond the particle's list
    E.upload_particle_orientation_lists([S.angles[:3]] + [S.angles[:2]] * (S.nMaps - 1), S.isQuat)
    with pytest.raises(RuntimeError, match="request 1") as e:
        E.ctf_scan(scan_requests([(0, 2, 0, 0), (S.nMaps - 1, 2, 0, 0)]), S.refCTF, S.ctfParam, own=True)
    assert e.value.rc == 2
    usable(E)
    E.close()
    # nothing uploaded: model, orientations, particles (the handle's CTF sets are not needed); every handle kind the same
    E2 = eng.Engine(to_engine_pd(S.pd), S.nMaps, S.nAngles, S.nCTF, algo=1, device=0)
    for step in (lambda: E2.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"]),
                 lambda: E2.upload_orientations(S.angles, S.isQuat),
                 lambda: E2.upload_particle_maps(S.maps)):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.ctf_scan(good, S.refCTF, S.ctfParam)
        assert e.value.rc == 2
        step()
    usable(E2)
    E2.close()
    for kw in (dict(shard=(2, 5)), dict(algo=2)):
        Ek = engine_for(S, kw.pop("algo", 1), **kw)
        usable(Ek)
        Ek.set_phase_timing(True)
        Ek.ctf_scan(good, S.refCTF, S.ctfParam)
        ph = Ek.phase_records()
        Ek.set_phase_timing(False)
        nB = -(-len(good) // Ek.max_batch()[0])  # a projection and a preparation per batch, a scan per launch
        count = [int((ph["phase"] == k).sum()) for k in range(3)]
        assert count[:2] == [nB, nB] and 1 <= count[2] <= nB and len(ph) == sum(count) and (ph["seconds"] > 0).all()
        Ek.close()


# ---- 7. own lists ----
def test_own_lists_against_the_oracle():
    """a round-2 handle: lists of different lengths, requests by list index, candidates off the grid"""
    case = "g8_n32_grid"
    S = setup(case)
    cand = doubled_setup(case)
    E = engine_for(S, 1)
    perm = [np.random.default_rng(60 + p).permutation(S.nAngles)[:S.nAngles - 3 * p] for p in range(S.nMaps)]
    assert len({len(q) for q in perm}) == S.nMaps
    E.upload_particle_orientation_lists([S.angles[q] for q in perm], S.isQuat)
    X = E.window_shifts()
    own, shared = [], []
    for p in range(S.nMaps):
        for k, (x, y) in ((0, (X[0], X[1])), (len(perm[p]) - 1, (X[-1], X[2]))):
            own.append((p, k, x, y))
            shared.append((p, int(perm[p][k]), x, y))
    a = E.ctf_scan(scan_requests(own), cand.refCTF, cand.ctfParam, own=True, want_cc=True, want_params=True)
    b = E.ctf_scan(scan_requests(shared), cand.refCTF, cand.ctfParam, want_cc=True, want_params=True)
    E.close()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    for k, (p, o, x, y) in enumerate(shared):
        want = oracle_scan(S, cand, p, o, int(x), int(y), X)
        ok = np.isfinite(want)
        assert ok.sum() >= cand.nCTF // 2 and within(a[0][k][ok], want[ok]).all(), (own[k], a[0][k], want)


# ---- the PSF kernels of a list (the host's transform runs on the device) ----
def test_psf_kernel_list_on_the_grid_triples_is_the_grid_bit_for_bit():
    from bioem_amd import ctf_scan as cs, hostlib
    P = load_case("g13_n32_psf_writectf")["P"]
    assert P["usepsf"]
    ref, par, _ = hostlib.psf_kernels(P["N"], P["pixelSize"], (P["startAmp"], P["endAmp"], P["nAmp"]),
                                      (P["startPhase"], P["endPhase"], P["nPhase"]), (P["startEnv"], P["endEnv"], P["nEnv"]))
    grid, _ = cs.refine_grid(P, 1)
    assert grid.tobytes() == par.tobytes() and np.abs(ref).max() > 0
    got = hostlib.ctf_kernel_list(P["N"], P["pixelSize"], par, usepsf=True)
    assert got.tobytes() == ref.tobytes()
    pick = [len(par) - 1, 0, 3]
    assert hostlib.ctf_kernel_list(P["N"], P["pixelSize"], par[pick], usepsf=True).tobytes() == ref[pick].tobytes()


# ---- 8. CLI ----
def test_cli_ctf_scan(tmp_path):
    """--CTFScan on a golden case: the files parse; at --CTFScanFactor 1 the candidates are the run's sets and the line of
    a particle's own best set carries, to the printed digits, the log posterior --BestWindow prints for its arg-max cell;
    Output_Probabilities is byte-identical to the run without the option; with --RefineOrientations FILE_Round2 appears"""
    from bioem_amd import best_window as bw, ctf_scan as cs, refine
    case = load_case("g10_n64")
    S = setup("g10_n64")
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    out = run_cli(inputs + ["--OutputFile", "out.txt", "--CTFScan", "scan1.txt", "--CTFScanFactor", "1", "--BestWindow",
                            "win.txt"], d, BIOEM_ALGO="1")
    assert "scan1.txt" in out
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    summ, cands, _ = cs.parse(str(d / "scan1.txt"))
    wsumm, cells, _ = bw.parse(str(d / "win.txt"))
    text = {ln.split()[1] + " " + ln.split()[2]: ln.split() for ln in open(d / "scan1.txt") if ln.startswith("CAND ")}
    wtext = {" ".join(ln.split()[1:4]): ln.split() for ln in open(d / "win.txt") if ln.startswith("CELL ")}
    om, _ = S.run(1)
    assert len(summ) == S.nMaps and (summ["G"] == S.nCTF).all()
    for p in range(S.nMaps):
        assert (summ[p]["orient"], summ[p]["shiftX"], summ[p]["shiftY"]) == (om[p]["orient"], om[p]["cent_x"], om[p]["cent_y"])
        assert summ[p]["orient"] == wsumm[p]["orient"] and (summ[p]["shiftX"], summ[p]["shiftY"]) == (wsumm[p]["peakX"],
                                                                                                     wsumm[p]["peakY"])
        c = int(om[p]["conv"])
        assert summ[p]["best"] == c  # the particle's own best set wins at its own best cell
        assert text["%d %d" % (p, c)][6] == wtext["%d %d %d" % (p, wsumm[p]["peakX"], wsumm[p]["peakY"])][4], p
        assert abs(cands[p]["weight"].sum() - 1) <= 1e-12
    out = run_cli(inputs + ["--OutputFile", "out4.txt", "--CTFScan", "scan4.txt"], d, BIOEM_ALGO="1")  # the default: 4-fold
    assert open(d / "out4.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    s4, c4, _ = cs.parse(str(d / "scan4.txt"))
    tr, cn = cs.refine_grid(case["P"], 4)
    assert (s4["G"] == len(tr)).all() and s4[0]["n"].tolist() == cn.tolist()
    every = np.arange(len(tr)).reshape(cn.tolist())[::1, ::4, ::4].ravel()
    for p in range(S.nMaps):  # every fourth candidate on the refined axes is a set of the run: the same line
        a, b = c4[p]["logp"][every], cands[p]["logp"]
        assert a.tobytes() == b.tobytes(), p
        assert np.isfinite(s4[p]["n_eff"]) and s4[p]["n_eff"] >= 1
    if S.isQuat:
        q = refine.local_grid(1, 0.05)
        with open(d / "grid.txt", "w") as f:
            f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
        run_cli(inputs + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--CTFScan", "scanr.txt",
                          "--CTFScanFactor", "2"], d, BIOEM_ALGO="1")
        assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
        s1, _, _ = cs.parse(str(d / "scanr.txt"))
        s2, c2, _ = cs.parse(str(d / "scanr.txt_Round2"))
        assert len(s1) == len(s2) == S.nMaps and (s2["G"] == s1["G"]).all() and np.isfinite(s2["logP"]).all()
