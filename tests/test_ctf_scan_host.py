"""CPU tests of the CTF scan's host side: ctf_kernel_list against the kernels of the run's set-up, the candidate rule of
--CTFScan (bioem_amd.ctf_scan.refine_grid and the CLI's ctf_scan_refine), derive on planted posteriors, the writer and the
parser of the text file, and the CLI's option handling.  No device: the PSF case of ctf_kernel_list transforms its kernels
on the device as the CLI's set-up does and lives in test_ctf_scan_gpu.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from golden_util import load_case, write_case_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")


def host_setup(name, d):
    from bioem_amd import hostlib
    case = load_case(name)
    write_case_inputs(case, d)
    return case, hostlib.setup_from_files(os.path.join(case["dir"], "param.txt"),
                                          os.path.join(str(d), "orient.txt") if case["orient_lines"] else None)


# ---- the kernels of a list of triples ----
@pytest.mark.parametrize("name", ["g8_n32_grid", "g10_n64", "g9_n35_odd"])
def test_kernel_list_on_the_grid_triples_is_the_grid_bit_for_bit(name, tmp_path):
    from bioem_amd import hostlib
    case, (S, _, ref, par) = host_setup(name, tmp_path)
    assert not S.usepsf and len(par) >= 2
    got = hostlib.ctf_kernel_list(S.pd.NumberPixels, S.pixelSize, par)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    # any order, any subset, repeats: a kernel depends on its triple alone
    pick = [len(par) - 1, 0, 0, len(par) // 2]
    assert hostlib.ctf_kernel_list(S.pd.NumberPixels, S.pixelSize, par[pick]).tobytes() == ref[pick].tobytes()
    with pytest.raises(ValueError):
        hostlib.ctf_kernel_list(S.pd.NumberPixels, S.pixelSize, par[:0])


def test_library_exports_header_and_request_layout():
    from bioem_amd import engine
    L = engine.load_library()
    for name in ("bioem_hip_ctf_scan", "bioem_hip_debug_ctf_scan"):
        assert hasattr(L, name) and name in engine.EXPORTS, name
    assert engine.SCAN_REQUEST_DTYPE.itemsize == 16
    assert engine.SCAN_REQUEST_DTYPE.names == ("particle", "orient", "shiftX", "shiftY")
    for f in ("ctf_scan", "best_match_ctf_scan", "debug_ctf_scan"):
        assert callable(getattr(engine.Engine, f))
    with open(os.path.join(ROOT, "include", "bioem_hip.h")) as f:
        hdr = f.read()
    assert "typedef struct { int particle, orient, shiftX, shiftY; } bioem_hip_scan_request;" in hdr
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)  # the declarations without their comments
    flat = re.sub(r"\s+", " ", flat)
    assert ("int bioem_hip_ctf_scan(bioem_hip_handle h, const bioem_hip_scan_request *req, int n, int ownLists, "
            "const float *kernels , const float *ctfParam3 , int G, double *logp_out , float *cc_out , "
            "bioem_hip_param5 *params_out );") in flat
    assert ("int bioem_hip_debug_ctf_scan(bioem_hip_handle h, const float *specP, const float *specRef, const float *sumRef, "
            "const float *sumsqRef, const int *shiftXY , int n, const float *kernels, const float *ctfParam3, int G, "
            "double *logp_out, float *cc_out, bioem_hip_param5 *params_out);") in flat


# ---- the candidates ----
@pytest.mark.parametrize("name", ["g8_n32_grid", "g10_n64", "g13_n32_psf_writectf"])
def test_refine_grid_keeps_the_grid_points_bit_for_bit(name, tmp_path):
    from bioem_amd import ctf_scan as cs, hostlib
    case, (S, _, _, par) = host_setup(name, tmp_path)
    P = case["P"]
    n = [P["nAmp"], P["nPhase"], P["nEnv"]]
    start, step, nn = cs.grid_of(P)
    grid, counts = cs.refine_grid(P, 1)
    assert counts.tolist() == n and grid.dtype == np.float32 and grid.shape == (int(np.prod(n)), 3)
    if not S.usepsf:  # (the host set-up makes the PSF grid on the device only)
        assert grid.tobytes() == par.tobytes()
    # the grid written out from the reference's loop: (float) i * step + start, amp outermost
    f = np.float32
    want = [[f(ia) * step[0] + start[0] if n[0] > 1 else start[0], f(ip) * step[1] + start[1] if n[1] > 1 else start[1],
             f(ie) * step[2] + start[2] if n[2] > 1 else start[2]]
            for ia in range(n[0]) for ip in range(n[1]) for ie in range(n[2])]
    assert grid.tobytes() == np.array(want, dtype=f).tobytes()
    for k in (2, 4, 8, 16):
        fine, cn = cs.refine_grid(P, k)
        assert cn.tolist() == [c * k if c > 1 else 1 for c in n]  # an axis with one point stays one point
        if len(fine) <= cs.MAX_CANDIDATES:  # (beyond it the CLI counts and refuses)
            cli, cn2 = hostlib.ctf_scan_refine(start, step, nn, k)
            assert cn2.tolist() == cn.tolist() and cli.tobytes() == fine.tobytes()
        every = fine.reshape(cn.tolist() + [3])[::k if n[0] > 1 else 1, ::k if n[1] > 1 else 1, ::k if n[2] > 1 else 1]
        assert every.reshape(-1, 3).tobytes() == grid.tobytes(), k
        # strictly ascending, inside the grid's range extended by one coarse step
        for a in range(3):
            v = np.unique(fine[:, a])
            assert len(v) == cn[a] and (n[a] == 1 or v[-1] < start[a] + n[a] * step[a])
    assert any(c == 1 for c in n) or name == "g13_n32_psf_writectf"
    for bad in (0, 3, 5, 32, -2):
        with pytest.raises(ValueError):
            cs.refine_grid(P, bad)
        with pytest.raises(ValueError):
            hostlib.ctf_scan_refine(start, step, nn, bad)


# ---- derive ----
COUNTS = [3, 8, 5]


def planted_triples():
    from bioem_amd import ctf_scan as cs
    start = np.array([0.1, 1000.0, 20.0], dtype=np.float32)
    step = np.array([0.1, 125.0, 30.0], dtype=np.float32)
    t, cn = cs.refine_grid((start, step, np.array(COUNTS, dtype=np.int32)), 1)
    assert cn.tolist() == COUNTS
    return t


def test_derive_delta_gives_its_candidate():
    from bioem_amd import ctf_scan as cs
    tr = planted_triples()
    G = len(tr)
    for g in (0, 57, G - 1):
        t = np.full(G, -np.inf)
        t[g] = -4321.5
        s, w, marg = cs.derive(t, tr)
        s = s[0]
        assert s["best"] == g and s["n_eff"] == 1 and s["logP"] == -4321.5 and s["skipped"] == G - 1 and s["G"] == G
        assert s["n"].tolist() == COUNTS
        for a in range(3):
            assert s["sd"][a] == 0 and s["mean"][a] == float(tr[g, a])
            i = np.unravel_index(g, COUNTS)[a]
            assert s["edge_mass"][a] == (1.0 if i in (0, COUNTS[a] - 1) else 0.0)
            assert marg[a][0, i] == 1 and marg[a].sum() == 1
        assert w[0, g] == 1 and w.sum() == 1


def test_derive_flat_table():
    from bioem_amd import ctf_scan as cs
    tr = planted_triples()
    G = len(tr)
    s, w, marg = cs.derive(np.full(G, 12.75), tr, COUNTS)
    s = s[0]
    assert abs(s["n_eff"] - G) <= 1e-12 * G and s["best"] == 0 and s["skipped"] == 0
    assert abs(s["logP"] - (12.75 + math.log(G))) <= 1e-13
    for a in range(3):
        assert abs(s["edge_mass"][a] - 2.0 / COUNTS[a]) <= 1e-14
        v = np.unique(tr[:, a]).astype(np.float64)
        assert abs(s["mean"][a] - v.mean()) <= 1e-12 * abs(v.mean()) and abs(s["sd"][a] - v.std()) <= 1e-12 * v.std()
    # an axis of one value carries all the mass on it
    one, _, _ = cs.derive(np.zeros(8), tr[:8], [1, 8, 1])
    assert one[0]["edge_mass"][0] == 1.0 and one[0]["sd"][0] == 0 and abs(one[0]["edge_mass"][1] - 0.25) <= 1e-14


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_derive_gaussian_in_one_axis(axis):
    """a discretised Gaussian along one axis, flat along the others: the mean and sd of that axis are those of the planted
    weights (formed here, in double), the other axes see their flat marginals"""
    from bioem_amd import ctf_scan as cs
    tr = planted_triples()
    v = np.unique(tr[:, axis]).astype(np.float64)
    mu, sig = v[len(v) // 2] + 0.3 * (v[1] - v[0]), 0.8 * (v[1] - v[0])
    lw = -0.5 * ((v - mu) / sig) ** 2
    idx = np.unravel_index(np.arange(len(tr)), COUNTS)[axis]
    s, w, marg = cs.derive(-2.0e4 + lw[idx], tr, COUNTS)
    s = s[0]
    pw = np.exp(lw - lw.max())
    pw /= pw.sum()
    mean = float((pw * v).sum())
    sd = math.sqrt(float((pw * (v - mean) ** 2).sum()))
    assert abs(s["mean"][axis] - mean) <= 1e-9 * abs(mean) and abs(s["sd"][axis] - sd) <= 1e-9 * sd
    assert abs(s["edge_mass"][axis] - (pw[0] + pw[-1])) <= 1e-12
    assert np.abs(marg[axis][0] - pw).max() <= 1e-14
    for a in range(3):
        if a != axis:
            assert abs(s["edge_mass"][a] - 2.0 / COUNTS[a]) <= 1e-13
    assert np.unravel_index(int(s["best"]), COUNTS)[axis] == int(np.argmax(pw))


def test_derive_skips_what_is_not_finite():
    from bioem_amd import ctf_scan as cs
    tr = planted_triples()
    G = len(tr)
    t = -100.0 + np.random.default_rng(4).uniform(-5, 0, G)
    t[[3, 40, 77]] = [np.nan, np.inf, -np.inf]
    s, w, _ = cs.derive(t, tr)
    assert s[0]["skipped"] == 3 and (w[0, [3, 40, 77]] == 0).all() and abs(w.sum() - 1) <= 1e-14
    s, w, _ = cs.derive(np.full(G, np.nan), tr)
    assert s[0]["best"] == -1 and s[0]["logP"] == -np.inf and np.isnan(s[0]["n_eff"]) and (w == 0).all()


# ---- writer / parser ----
def test_writer_and_parser_round_trip(tmp_path):
    from bioem_amd import ctf_scan as cs, hostlib
    tr = planted_triples()
    G = len(tr)
    rng = np.random.default_rng(12)
    t = -3.0e4 + rng.uniform(-30.0, 0.0, (4, G))
    t[1, 5] = np.nan
    t[2] = -np.inf
    t[2, G - 1] = -12.5
    orient = np.array([3, 0, 17, -1])
    sx, sy = np.array([2, -5, 0, 0]), np.array([-1, 4, 31, 0])
    numconst = np.array([-1000.5, -1000.5, 7.0, 0.0])
    path = str(tmp_path / "scan.txt")
    lam = 0.019866
    hostlib.write_ctf_scan(path, t, tr, COUNTS, orient, sx, sy, numconst, usepsf=False, elecwavel=lam)
    summ, cands, notation = cs.parse(path)
    assert len(summ) == 4 and "CAND" in notation and "edgeMass" in notation and "defocus" in notation
    want, W, _ = cs.derive(t[:3] + numconst[:3, None], tr, COUNTS)
    unit = np.array([1.0, float(np.float32(1) / np.float32(2)) / math.pi / float(np.float32(lam)) * 0.0001, 1.0])

    def close(a, b, what):
        a, b = np.float64(a), np.float64(b)
        assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 1e-12 * max(abs(b), 1e-3), (what, a, b)

    for p in range(3):
        s = summ[p]
        assert (s["orient"], s["shiftX"], s["shiftY"], s["best"]) == (orient[p], sx[p], sy[p], want[p]["best"])
        assert s["G"] == G and s["n"].tolist() == COUNTS and s["skipped"] == want[p]["skipped"]
        close(s["logP"], want[p]["logP"], "logP")
        close(s["n_eff"], want[p]["n_eff"], "n_eff")
        for a in range(3):
            close(s["mean"][a], want[p]["mean"][a] * unit[a], ("mean", a))
            close(s["sd"][a], want[p]["sd"][a] * unit[a], ("sd", a))
            close(s["edge_mass"][a], want[p]["edge_mass"][a], ("edge", a))
        b = tr[int(want[p]["best"])].astype(np.float64)
        close(s["amp"], b[0], "amp")
        close(s["pha"], b[1] * unit[1], "pha")
        close(s["env"], b[2], "env")
        c = cands[p]
        ok = np.isfinite(t[p])
        assert (np.isfinite(c["logp"]) == ok).all()
        assert (np.abs(c["logp"][ok] - (t[p] + numconst[p])[ok]) <= 1e-12 * np.abs(t[p][ok])).all()
        assert (np.abs(c["weight"] - W[p]) <= 1e-12).all()
        assert (np.abs(c["amp"] - tr[:, 0]) <= 1e-12).all() and (np.abs(c["env"] - tr[:, 2]) <= 1e-10).all()
        assert (np.abs(c["pha"] - tr[:, 1].astype(np.float64) * unit[1]) <= 1e-12 * np.abs(c["pha"])).all()
    assert summ[3]["orient"] == -1 and summ[3]["G"] == 0 and cands[3]["logp"].size == 0
    assert summ[1]["skipped"] == 1 and summ[2]["skipped"] == G - 1 and summ[2]["n_eff"] == 1.0
    # PSF columns and statistics are printed as they are
    hostlib.write_ctf_scan(path, t, tr, COUNTS, orient, sx, sy, 0.0, usepsf=True)
    s2, _, note2 = cs.parse(path)
    want2, _, _ = cs.derive(t[:1], tr, COUNTS)
    assert "PSF" in note2 and abs(s2[0]["mean"][1] - want2[0]["mean"][1]) <= 1e-12 * abs(want2[0]["mean"][1])
    with pytest.raises(ValueError, match="Opening"):
        hostlib.write_ctf_scan(str(tmp_path / "no_such_dir" / "x.txt"), t, tr, COUNTS, orient, sx, sy, numconst)
    text = open(path).read()
    for bad in ("SCAN 0 1 2 3\n", text.replace("CAND 0 0 ", "CAND 9 0 ", 1), text.replace("CAND 1 5 ", "BAND 1 5 "),
                text.replace("CAND 0 1 ", "CAND 0 2 ", 1), "\n".join(text.split("\n")[:-3]) + "\n",
                text.replace(cs.BAR, "****", 1)):
        (tmp_path / "bad.txt").write_text(bad)
        with pytest.raises(ValueError):
            cs.parse(str(tmp_path / "bad.txt"))


# ---- the CLI's option handling (nothing here reaches a device) ----
def run(args, d):
    return subprocess.run([EXE] + args, cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


def test_cli_names_the_options(tmp_path):
    r = run(["--help"], tmp_path)
    assert "--CTFScan arg" in r.stdout and "--CTFScanFactor arg" in r.stdout and "1, 2, 4, 8 or 16 (default 4)" in r.stdout
    r = run(["--Modelfile", "m.txt", "--CTFScan"], tmp_path)
    assert "requires an argument" in r.stdout and "Command line inputs" in r.stdout and "Running" not in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "none.txt", "--PrintBestCalMap", "best.txt", "--CTFScan", "scan.txt"], tmp_path)
    assert r.returncode != 0 and "--PrintBestCalMap goes without" in r.stdout and "--CTFScan" in r.stdout
    assert not (tmp_path / "scan.txt").exists()


def test_cli_refuses_a_bad_factor_and_too_many_candidates_without_a_run(tmp_path):
    param = os.path.join(load_case("g10_n64")["dir"], "param.txt")
    base = ["--Inputfile", param, "--Modelfile", "no_model.txt", "--Particlesfile", "no_particles.txt", "--ReadOrientation",
            "no_orientations.txt"]
    for bad in ("3", "0", "32", "-4", "4x", ""):
        r = run(base + ["--CTFScan", "scan.txt", "--CTFScanFactor", bad], tmp_path)
        assert "--CTFScanFactor needs one of 1, 2, 4, 8, 16" in r.stdout, (bad, r.stdout[-500:])
        assert "Command line inputs" in r.stdout and "--CTFScan arg" in r.stdout  # the usage text, as for a bad option
        assert "READING BioEM PARAMETERS" not in r.stdout and "Running" not in r.stdout
    r = run(base + ["--CTFScanFactor", "2"], tmp_path)
    assert r.returncode != 0 and "--CTFScanFactor goes with --CTFScan" in r.stdout
    # 6 x 7 x 5 sets refined 8-fold are 48 x 56 x 40 = 107 520 candidates; 2-fold 12 x 14 x 10 = 1 680 pass this check
    big = tmp_path / "big.txt"
    big.write_text(open(param).read().replace("CTF_B_ENV 20.0 200.0 3", "CTF_B_ENV 20.0 200.0 5")
                   .replace("CTF_DEFOCUS 1.0 3.0 2", "CTF_DEFOCUS 1.0 3.0 7")
                   .replace("CTF_AMPLITUDE 0.1 0.1 1", "CTF_AMPLITUDE 0.1 0.4 6"))
    args = ["--Inputfile", str(big)] + base[2:] + ["--CTFScan", "s.txt"]
    r = run(args + ["--CTFScanFactor", "8"], tmp_path)
    assert r.returncode != 0 and "107520 candidate CTF sets" in r.stdout and "48 x 56 x 40" in r.stdout, r.stdout[-800:]
    assert "4096" in r.stdout and not (tmp_path / "s.txt").exists()
    r = run(args + ["--CTFScanFactor", "2"], tmp_path)  # passes the count and ends at the particle file that is not there
    assert r.returncode != 0 and "candidate CTF sets" not in r.stdout
    assert not (tmp_path / "s.txt").exists()
