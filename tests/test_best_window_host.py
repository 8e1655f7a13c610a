"""CPU tests of the window posterior's host side: the displacement sets of bioem_hip_window_count / _offsets against the
lists written out from the reference's loops, the C ABI, bioem_amd.best_window (derive, marginal, parse), the writer of
--BestWindow, the CLI's option handling, and tests/window_reference.py pinned to the CPU oracle.  No device."""
import ctypes as C
import math
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import window_reference as wr
from golden_util import load_case, oracle_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_TOL, ABS_TOL = 1e-4, 2e-2  # the project's figures against the oracle (test_gpu_parity.py)


@pytest.mark.parametrize("N", [8, 32, 35, 64])
def test_window_sets_against_the_written_out_lists(N):
    from bioem_amd import engine
    L = engine.load_library()
    seen = 0
    for maxD in list(range(8)) + [20]:
        for grid in (1, 2, 3):
            for algo in (1, 2):
                if maxD >= N // 2:
                    assert L.bioem_hip_window_count(N, maxD, grid, algo) <= 0, (N, maxD, grid, algo)
                    with pytest.raises(ValueError):
                        engine.window_offsets(N, maxD, grid, algo)
                    continue
                want = wr.offsets(N, maxD, grid, algo)
                got = engine.window_offsets(N, maxD, grid, algo)
                assert got.dtype == np.int32 and got.tolist() == want.tolist(), (N, maxD, grid, algo, got, want)
                assert L.bioem_hip_window_count(N, maxD, grid, algo) == len(want)
                assert (np.diff(got) > 0).all()
                # a short buffer is filled as far as it goes and the count still comes back
                buf = np.full(len(want) + 2, 12345, dtype=np.int32)
                assert L.bioem_hip_window_offsets(N, maxD, grid, algo, buf.ctypes.data_as(C.c_void_p), 1) == len(want)
                assert buf[0] == want[0] and (buf[1:] == 12345).all()
                seen += 1
    assert seen >= 12
    assert engine.window_offsets(32, 5, 2, 1).tolist() == [-4, -2, 0, 1, 3, 5]
    assert engine.window_offsets(32, 5, 2, 2).tolist() == [-3, -1, 1, 3, 5]  # 2 (maxD / grid) + 1 cells from -maxD


def test_window_count_refuses_invalid_arguments():
    from bioem_amd import engine
    L = engine.load_library()
    for args in [(0, 0, 1, 1), (-4, 1, 1, 1), (32, 5, 0, 1), (32, 5, -1, 2), (32, 16, 1, 1), (32, 40, 1, 2), (35, 17, 1, 1),
                 (32, -1, 1, 1), (32, 5, 1, 0), (32, 5, 1, 3)]:
        assert L.bioem_hip_window_count(*args) <= 0, args
        assert L.bioem_hip_window_offsets(*args, None, 0) <= 0, args
    assert L.bioem_hip_window_count(35, 16, 1, 1) == 33


def test_library_exports_header_and_request_layout():
    from bioem_amd import engine
    L = engine.load_library()
    names = ("bioem_hip_window_count", "bioem_hip_window_offsets", "bioem_hip_window_posterior", "bioem_hip_debug_window")
    for name in names:
        assert hasattr(L, name) and name in engine.EXPORTS, name
    assert engine.WINDOW_REQUEST_DTYPE.itemsize == 12 and engine.WINDOW_REQUEST_DTYPE.names == ("particle", "orient", "conv")
    for f in ("window_posterior", "best_match_window", "debug_window"):
        assert callable(getattr(engine.Engine, f))
    with open(os.path.join(ROOT, "include", "bioem_hip.h")) as f:
        hdr = f.read()
    assert "typedef struct { int particle, orient, conv; } bioem_hip_window_request;" in hdr
    assert "int bioem_hip_window_count(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo);" in hdr
    assert ("int bioem_hip_window_offsets(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, "
            "int *shifts, int cap);") in hdr
    assert re.search(r"int bioem_hip_window_posterior\(bioem_hip_handle h, const bioem_hip_window_request \*req, int n, "
                     r"int ownLists,\s+double \*logp_out[^,]*,\s*float \*cc_out[^,]*,\s+bioem_hip_param5 \*params_out", hdr)
    assert re.search(r"int bioem_hip_debug_window\(bioem_hip_handle h, const float \*specConv, const float \*specRef, "
                     r"const bioem_hip_param5 \*params,\s+const float \*sumRef, const float \*sumsqRef, int n, "
                     r"double \*logp_out, float \*cc_out\);", hdr)


# ---- derive / marginal ----
SYM = np.array([-4, -2, 0, 2, 4])
IRR = np.array([-4, -2, 0, 1, 3, 5])


@pytest.mark.parametrize("X,i,j,edge", [(SYM, 2, 2, 0.0), (SYM, 0, 3, 1.0), (IRR, 3, 5, 1.0), (IRR, 1, 4, 0.0)])
def test_derive_one_finite_cell(X, i, j, edge):
    from bioem_amd import best_window as bw
    t = np.full((len(X), len(X)), -np.inf)
    t[i, j] = -1234.5
    s, w = bw.derive(t, X)
    s = s[0]
    assert s["logP"] == -1234.5 and s["peakLogp"] == -1234.5 and (s["peakX"], s["peakY"]) == (X[i], X[j])
    assert (s["meanX"], s["meanY"]) == (X[i], X[j]) and s["sdX"] == 0 and s["sdY"] == 0
    assert s["n_eff"] == 1 and s["edge_mass"] == edge and s["skipped"] == len(X) ** 2 - 1 and s["nd"] == len(X)
    assert w[0, i, j] == 1 and w.sum() == 1


def test_derive_flat_table_on_a_symmetric_set():
    from bioem_amd import best_window as bw
    nd = len(SYM)
    s, w = bw.derive(np.full((nd, nd), 77.25), SYM)
    s = s[0]
    assert abs(s["meanX"]) < 1e-15 and abs(s["meanY"]) < 1e-15
    assert abs(s["n_eff"] - nd * nd) < 1e-12 * nd * nd
    assert abs(s["edge_mass"] - (4 * nd - 4) / nd ** 2) < 1e-15
    assert abs(s["logP"] - (77.25 + math.log(nd * nd))) < 1e-13
    assert abs(s["sdX"] - math.sqrt(np.mean(SYM.astype(float) ** 2))) < 1e-14 and s["skipped"] == 0
    assert (s["peakX"], s["peakY"]) == (SYM[0], SYM[0])  # the first among equals, row-major


def mp_table_stats(t, X):
    """logP, means and edge mass of the finite cells in mpmath"""
    with mpmath.workprec(400):
        cells = [(i, j, mpmath.mpf(float(t[i, j]))) for i in range(len(X)) for j in range(len(X)) if np.isfinite(t[i, j])]
        m = max(c[2] for c in cells)
        tot = sum(mpmath.exp(c[2] - m) for c in cells)
        logP = m + mpmath.log(tot)
        mx = sum(mpmath.exp(c[2] - m) * int(X[c[0]]) for c in cells) / tot
        my = sum(mpmath.exp(c[2] - m) * int(X[c[1]]) for c in cells) / tot
        lo, hi = int(X.min()), int(X.max())
        edge = sum(mpmath.exp(c[2] - m) for c in cells if int(X[c[0]]) in (lo, hi) or int(X[c[1]]) in (lo, hi)) / tot
        neff = tot * tot / sum(mpmath.exp(2 * (c[2] - m)) for c in cells)
        return float(logP), float(mx), float(my), float(edge), float(neff)


def test_derive_against_mpmath_with_a_spread_of_1400_log_units_and_skipped_cells():
    from bioem_amd import best_window as bw
    rng = np.random.default_rng(5)
    nd = len(IRR)
    t = -3.0e4 + rng.uniform(-1400.0, 0.0, (3, nd, nd))
    t[0, 2, 3] = t[0].max() + 0.25        # a clear peak
    t[1, 0, 0], t[1, 4, 1], t[1, 5, 5] = np.nan, np.inf, -np.inf  # skipped and counted
    t[2] = -2.5e4 + rng.uniform(-3.0, 0.0, (nd, nd))  # a broad posterior
    s, w = bw.derive(t, IRR)
    assert s["skipped"].tolist() == [0, 3, 0]
    for k in range(3):
        logP, mx, my, edge, neff = mp_table_stats(t[k], IRR)
        assert abs(s[k]["logP"] - logP) <= 4 * np.spacing(abs(logP)), (k, s[k]["logP"], logP)
        assert abs(s[k]["meanX"] - mx) <= 1e-13 and abs(s[k]["meanY"] - my) <= 1e-13
        assert abs(s[k]["edge_mass"] - edge) <= 1e-13 and abs(s[k]["n_eff"] - neff) <= 1e-12 * neff
        assert abs(w[k].sum() - 1) <= 1e-14 and (w[k][~np.isfinite(t[k])] == 0).all()
    assert (s[0]["peakX"], s[0]["peakY"]) == (IRR[2], IRR[3])
    # no finite cell at all
    s, w = bw.derive(np.full((nd, nd), np.nan), IRR)
    assert s[0]["logP"] == -np.inf and s[0]["skipped"] == nd * nd and np.isnan(s[0]["n_eff"]) and (w == 0).all()


def test_marginal_is_the_log_sum_exp_cell_by_cell():
    from bioem_amd import best_window as bw
    rng = np.random.default_rng(9)
    K, nd = 7, 5
    t = -2.0e4 + rng.uniform(-900.0, 0.0, (K, nd, nd))
    t[3, 1, 1] = np.nan
    t[:, 4, 4] = -np.inf
    got = bw.marginal(t)
    assert got[4, 4] == -np.inf
    with mpmath.workprec(400):
        for i in range(nd):
            for j in range(nd):
                v = [mpmath.mpf(float(x)) for x in t[:, i, j] if np.isfinite(x)]
                if not v:
                    continue
                m = max(v)
                want = float(m + mpmath.log(sum(mpmath.exp(x - m) for x in v)))
                assert abs(got[i, j] - want) <= 4 * np.spacing(abs(want)), (i, j, got[i, j], want)


# ---- writer / parser ----
def test_writer_and_parser_round_trip(tmp_path):
    from bioem_amd import best_window as bw, hostlib
    rng = np.random.default_rng(11)
    nd = len(IRR)
    t = -3.0e4 + rng.uniform(-40.0, 0.0, (4, nd, nd))
    t[1, 2, 2] = np.nan
    t[2] = -np.inf
    t[2, 5, 0] = -12.5
    orient = np.array([3, 0, 17, -1])
    conv = np.array([1, 0, 2, 0])
    ctf = np.array([[0.1, 2.5, 100.0], [0.2, 1.25, 50.0], [0.3, 0.5, 0.0]], dtype=np.float32)
    numconst = np.array([-1000.5, -1000.5, 7.0, 0.0])
    path = str(tmp_path / "win.txt")
    hostlib.write_best_window(path, t, IRR, orient, conv, ctf, numconst, usepsf=False, elecwavel=0.019866)
    summ, cells, notation = bw.parse(path)
    assert len(summ) == 4 and "CELL" in notation and "edgeMass" in notation
    want, W = bw.derive(t[:3] + numconst[:3, None, None], IRR)

    def close(a, b, what):
        a, b = np.float64(a), np.float64(b)
        assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 1e-12 * max(abs(b), 1e-3), (what, a, b)

    for p in range(3):
        for f in bw.STAT_FIELDS:
            close(summ[p][f], want[p][f], (p, f))
        assert summ[p]["orient"] == orient[p] and summ[p]["nd"] == nd
        close(summ[p]["amp"], ctf[conv[p], 0], "amp")
        close(summ[p]["pha"], float(ctf[conv[p], 1] / np.float32(2)) / math.pi / float(np.float32(0.019866)) * 0.0001, "pha")
        close(summ[p]["env"], ctf[conv[p], 2], "env")
        c = cells[p]
        assert (c["X"] == IRR[:, None]).all() and (c["Y"] == IRR[None, :]).all()
        ok = np.isfinite(t[p])
        assert (np.abs(c["logp"][ok] - (t[p] + numconst[p])[ok]) <= 1e-12 * np.abs(t[p][ok])).all()
        assert (np.isfinite(c["logp"]) == ok).all()
        assert (np.abs(c["weight"] - W[p]) <= 1e-12).all()
    assert summ[3]["orient"] == -1 and summ[3]["nd"] == 0 and cells[3]["logp"].size == 0
    assert summ[1]["skipped"] == 1 and summ[2]["skipped"] == nd * nd - 1 and summ[2]["edge_mass"] == 1.0
    # PSF columns are printed as they are
    hostlib.write_best_window(path, t, IRR, orient, conv, ctf, 0.0, usepsf=True)
    s2, _, note2 = bw.parse(path)
    assert "PSF" in note2 and abs(s2[0]["pha"] - float(ctf[1, 1])) <= 1e-12
    with pytest.raises(ValueError, match="Opening"):
        hostlib.write_best_window(str(tmp_path / "no_such_dir" / "x.txt"), t, IRR, orient, conv, ctf, numconst)
    text = open(path).read()
    for bad in ("WINDOW 0 1 2 3\n", text.replace("CELL 0 -4 -4", "CELL 9 -4 -4", 1), text.replace("CELL 1 5 5", "BELL 1 5 5"),
                "\n".join(text.split("\n")[:-3]) + "\n", text.replace(bw.BAR, "****", 1)):
        (tmp_path / "bad.txt").write_text(bad)
        with pytest.raises(ValueError):
            bw.parse(str(tmp_path / "bad.txt"))


def test_cli_names_the_option_and_refuses_it_without_a_file(tmp_path):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,  # noqa: E731
                                      text=True, timeout=60)
    r = run(["--help"])
    assert "--BestWindow" in r.stdout and "_Round2" in r.stdout
    r = run(["--Modelfile", "m.txt", "--BestWindow"])
    assert "requires an argument" in r.stdout and "Command line inputs" in r.stdout and "Running" not in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "none.txt", "--PrintBestCalMap", "best.txt", "--BestWindow", "win.txt"])
    assert r.returncode != 0 and "--PrintBestCalMap goes without" in r.stdout and "--BestWindow" in r.stdout
    assert not (tmp_path / "win.txt").exists()


# ---- the reference pinned to the oracle ----
@pytest.mark.parametrize("case,algo", [("g3_n32_trace", 1), ("g3_n32_trace", 2), ("g8_n32_grid", 1), ("g8_n32_grid", 2)])
def test_reference_against_the_oracle_comparison(case, algo):
    """for one (orientation, CTF) pair and every particle: the arg-max cell of the reference table is the shift
    orc_compare reports, and the log-sum-exp over the cells is its log(Total) + Constoadd"""
    import oracle as orc
    S = oracle_setup(load_case(case))
    X = wr.offsets(S.N, S.pd.maxDisplaceCenter, S.pd.GridSpaceCenter, algo)
    o, c = S.nAngles // 2, S.nCTF - 1
    conv, p5 = S.conv_spectra(o)
    pmap, _ = S.new_prob()
    pd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(pd, f, getattr(S.pd, f))
    pd.writeAngles = 0
    S.pd, keep = pd, S.pd
    try:
        S.compare(algo, o, c, conv[c:c + 1], p5[c:c + 1], pmap)
    finally:
        S.pd = keep
    for p in range(S.nMaps):
        t, _ = wr.table(pd, conv[c], S.refFFT[p], p5[c], S.sumRef[p], S.sumsqRef[p], X)
        i, j = np.unravel_index(int(np.argmax(t)), t.shape)
        rec = pmap[p]
        assert (rec["orient"], rec["conv"]) == (o, c)
        assert (X[i], X[j]) == (rec["cent_x"], rec["cent_y"]), (p, X[i], X[j], rec)
        have, want = wr.lse(t), math.log(rec["Total"]) + rec["Constoadd"]
        assert abs(have - want) <= max(ABS_TOL, REL_TOL * abs(want)), (p, have, want)
