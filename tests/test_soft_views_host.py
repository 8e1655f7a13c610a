"""CPU tests of the posterior-weighted view sums' host side: the exact reference (tests/soft_view_reference.py) against
brute force over one pseudo-particle per cell and against the ordered float64 restatement of the kernels' arithmetic, and
bioem_amd/soft_views.py (cell parameters, posterior weights, members, requests, the text lines of --ReconstructSoft)."""
import os
import subprocess

import numpy as np
import pytest

import soft_view_reference as sr
import view_reference as vr
import window_reference as wr
from golden_util import load_case, oracle_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_engine_methods():
    from bioem_amd import engine
    L = engine.load_library()
    for name in ("bioem_hip_view_sums_soft", "bioem_hip_debug_view_sums_soft", "bioem_hip_reconstruct_soft"):
        assert hasattr(L, name) and name in engine.EXPORTS, name
    for name in ("view_sums_soft", "debug_view_sums_soft", "reconstruct_soft", "soft_members"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.SOFT_MEMBER_DTYPE.itemsize == 40 and sr.MEMBER_DTYPE == engine.SOFT_MEMBER_DTYPE


def hand_made(N):
    """three particles, two CTF sets, members with float32-valued tables over the shifts (-2, 0, 3, N - 1)"""
    H = N // 2 + 1
    k1, k2 = np.arange(N)[:, None], np.arange(H)[None, :]
    spec = np.stack([(1 + k1 + 2 * k2) + 1j * (k1 - k2), (3 - k1) + 1j * (0.5 * k2 + 1), (k1 * k2 % 5) - 2j * (k1 % 3)])
    ctf = np.stack([(1 + 0.25 * k1) + 1j * (0.5 * k2 - 0.125 * k1), (2 - 0.5 * k2) + 1j * (0.25 * k1 * (k2 % 2))])
    shifts = np.array([-2, 0, 3, N - 1], dtype=np.int32)
    nd = len(shifts)
    i, j = np.arange(nd)[:, None], np.arange(nd)[None, :]
    plan = [(0, 0, 0), (1, 0, 1), (2, 1, 0), (1, 1, 1), (0, 2, 1)]
    cells = np.stack([((i + 2 * j + r) % 5 - 2) * 0.25 * (1 + r) for r in range(len(plan))]).astype(np.float64)
    mus = np.stack([((2 * i + j + r) % 4 - 1.5) * 0.5 for r in range(len(plan))])
    mem = np.zeros(len(plan), dtype=sr.MEMBER_DTYPE)
    for r, (p, g, c) in enumerate(plan):
        mem[r]["particle"], mem[r]["group"], mem[r]["conv"] = p, g, c
        mem[r]["s2"] = (cells[r] ** 2).sum()
        mem[r]["b"] = (cells[r] * mus[r]).sum()
        mem[r]["mass"] = 0.25 * (r + 1)
    return spec.astype(np.complex64), ctf.astype(np.complex64), mem, cells, mus, shifts, 4


@pytest.mark.parametrize("N", [8, 9])
def test_exact_reference_against_brute_force(N):
    """view_reference.numpy_sums over nd^2 pseudo-particles per member, one per cell with norm = a, weight 1 and the cell's
    mu, computes the same sums in float64: T = nd^2 n_g terms of a handful of roundings each, so within 8 (T + 16) 2^-53
    of sum |term|.  The scale of the soft bound (sum |a| in place of |W|) bounds that sum from above."""
    spec, ctf, mem, cells, mus, shifts, nG = hand_made(N)
    ex = sr.exact_sums(spec, ctf, mem, cells, shifts, nG)
    S, rec, grp = sr.brute_force(spec, mem, cells, mus, shifts)
    num, den, stats = vr.numpy_sums(S, ctf, rec, None, grp, nG)
    an, ad, size = sr.scales(spec, ctf, mem, cells, nG)
    assert size.tolist() == [2, 2, 1, 0] and np.array_equal(ex[4][:, 0], size) and np.array_equal(stats[:, 0], size * 16)
    assert np.array_equal(ex[4][:, 1], [0.75, 1.75, 1.25, 0.0])
    T = (16 * size)[:, None, None]
    en, ed = sr.errors(num, den, ex)
    # |b| <= sum |a| |mu| is not what the scale holds: bound the brute-force offset by its own terms
    an_b = an.copy()
    for r, m in enumerate(mem):
        K = np.abs(vr.hermitian_kernel(vr.as_complex(ctf)[int(m["conv"])]))
        an_b[int(m["group"]), 0, 0] += K[0, 0] * (np.abs(cells[r] * mus[r]).sum() - abs(float(m["b"]))) * N * N
    assert (en <= 8 * (T + 16) * sr.U * an_b).all() and (ed <= 8 * (T + 16) * sr.U * ad).all()
    assert not ex[0][3].any() and not ex[2][3].any() and ex[0][:3].any()
    # the float64 restatement of the definition, and the ordered restatement of the kernels to the kernels' bound
    num2, den2, stats2 = sr.numpy_sums(spec, ctf, mem, cells, shifts, nG)
    en, ed = sr.errors(num2, den2, ex)
    assert (en <= 8 * (T + 16) * sr.U * an).all() and (ed <= 8 * (T + 16) * sr.U * ad).all()
    assert np.array_equal(stats2, ex[4])
    bn, bd = sr.bounds(an, ad, size, len(shifts))
    en, ed = sr.errors(*sr.ordered_sums(spec, ctf, mem, cells, shifts, nG), ex)
    assert (sr.ratios(en, bn) <= 1.0).all() and (sr.ratios(ed, bd) <= 1.0).all()


def test_one_hot_member_is_a_member_of_the_hard_sums():
    """the exact soft sums of one-hot tables are the exact hard sums of view_reference.exact_sums"""
    N = 9
    spec, ctf, mem, _, _, _, nG = hand_made(N)
    shifts = np.array([4, -8, 0], dtype=np.int32)
    rec = np.zeros(3, dtype=[("cent_x", "<i4"), ("cent_y", "<i4"), ("conv", "<i4"), ("norm", "<f4"), ("mu", "<f4")])
    rec["cent_x"], rec["cent_y"], rec["conv"] = [4, -8, 0], [0, 4, -8], [0, 1, 1]
    rec["norm"], rec["mu"] = [1.5, -0.75, 2.0], [0.25, 3.0, -1.0]
    w = np.array([1.0, 0.5, 2.0])
    g = np.array([0, 1, 0], dtype=np.int32)
    m = np.zeros(3, dtype=sr.MEMBER_DTYPE)
    cells = np.zeros((3, 3, 3))
    for p in range(3):
        a = w[p] * float(rec[p]["norm"])
        cells[p, list(shifts).index(rec[p]["cent_x"]), list(shifts).index(rec[p]["cent_y"])] = a
        m[p] = (p, g[p], rec[p]["conv"], 0, a * float(rec[p]["norm"]), a * float(rec[p]["mu"]), w[p])
    hard = vr.exact_sums(spec, ctf, rec, w, g, 2)
    soft = sr.exact_sums(spec, ctf, m, cells, shifts, 2)
    for k in (0, 2, 4):   # the correctly rounded values
        assert np.array_equal(hard[k], soft[k]), k
    for k in (1, 3):      # the rests: the soft reference multiplies two rounded twiddles, 2^-160 of a term apart
        assert (np.abs(hard[k] - soft[k]) <= 2.0 ** -150 * np.abs(hard[k - 1]).max()).all(), k


@pytest.mark.parametrize("N,nd", [(32, 1), (32, 2), (35, 3), (37, 21), (32, 32), (35, 35)])
def test_ordered_arithmetic_stays_within_the_bound_on_the_rounded_class(N, nd):
    """the inputs of the GPU tests' rounded class: the float64 restatement of the kernels' arithmetic (the library's
    twiddles, every product and sum rounded once in the stated order) against the exact sums, to the derived bound"""
    ctf = sr.random_complex(4, N, 5 * N + nd, 1.5)
    spec, mem, cells, shifts, nG = sr.rounded_problem(N, nd, 4, 100 * N + nd)
    assert len(shifts) == nd and abs(shifts).max() == N - 1
    ex = sr.exact_sums(spec, ctf, mem, cells, shifts, nG)
    an, ad, size = sr.scales(spec, ctf, mem, cells, nG)
    assert size.tolist() == [4, 1, 0, 3]
    bn, bd = sr.bounds(an, ad, size, nd)
    en, ed = sr.errors(*sr.ordered_sums(spec, ctf, mem, cells, shifts, nG), ex)
    rn, rd = sr.ratios(en, bn), sr.ratios(ed, bd)
    print("ordered N=%d nd=%d: worst |num - exact| / bound = %.3g, |den - exact| / bound = %.3g" % (N, nd, rn.max(), rd.max()))
    assert (rn <= 1.0).all() and (rd <= 1.0).all()
    if nd > 1:   # the tables cancel: |W| at k = 0 is far below sum |a|
        assert abs(cells[0].sum()) < 1e-9 * np.abs(cells[0]).sum()


@pytest.mark.parametrize("nd", [1, 3, 5])
def test_ordered_arithmetic_is_exact_on_the_exact_class(nd):
    ctf = sr.integer_kernels(3, 32, nd)
    spec, mem, cells, shifts, nG = sr.exact_problem(nd, [0, 1, 7, 3, 2], 3, 40 + nd)
    # a particle in three groups (the members of a group are of different particles), a particle without a member
    assert max(np.bincount(mem["particle"])) >= 3 and len(spec) - 1 not in mem["particle"]
    ex = sr.exact_sums(spec, ctf, mem, cells, shifts, nG)
    assert not ex[1].any() and not ex[3].any()   # representable: nothing left over
    num, den = sr.ordered_sums(spec, ctf, mem, cells, shifts, nG)
    assert num.tobytes() == ex[0].tobytes() and den.tobytes() == ex[2].tobytes()


# ---- bioem_amd/soft_views.py ----
def planted(n_req, nd, seed):
    from bioem_amd import engine as eng
    rng = np.random.default_rng(seed)
    req = np.zeros(n_req, dtype=eng.WINDOW_REQUEST_DTYPE)
    logp = rng.standard_normal((n_req, nd, nd)) * 3.0 - 50.0
    cc = (rng.standard_normal((n_req, nd, nd)) * 0.1 + 1.0).astype(np.float32)
    par = np.zeros(n_req, dtype=eng.PARAM5_DTYPE)
    par["sumC"] = rng.standard_normal(n_req) * 5.0
    par["sumsquareC"] = rng.random(n_req) * 100.0 + 500.0
    return req, logp, cc, par


def test_cell_params_solve_the_least_squares_problem():
    """norm and mu of a cell minimise sum (R - norm C - mu)^2 given sum C, sum C^2, sum R and cc = sum R C: the normal
    equations  norm sumsqC + mu sumC = cc,  norm sumC + mu Ntotpi = sumR  hold to rounding"""
    from bioem_amd import soft_views as sv
    N = 12
    req, logp, cc, par = planted(3, 4, 1)
    sums = np.array([3.0, -2.0, 0.5], dtype=np.float32)
    norm, mu = sv.cell_params(cc, par, sums, N)
    sC, s2C = par["sumC"].astype(np.float64)[:, None, None], par["sumsquareC"].astype(np.float64)[:, None, None]
    r1 = norm * s2C + mu * sC - cc.astype(np.float64)
    r2 = norm * sC + mu * float(N * N) - sums.astype(np.float64)[:, None, None]
    scale = np.abs(norm) * s2C + np.abs(mu) * (np.abs(sC) + N * N)
    assert (np.abs(r1) <= 16 * sr.U * scale).all() and (np.abs(r2) <= 16 * sr.U * scale).all()


@pytest.mark.parametrize("name", ["g10_n64", "g9_n35_odd"])
def test_cell_params_against_the_oracle_at_the_arg_max_cell(name):
    """norm and mu of the oracle's best record against cell_params at that record's cell, with cc from the float64 c2r of
    the oracle's own conv and particle spectra (tests/window_reference.py): the oracle evaluates the expression in float
    from its float cc, so to the project's end-to-end figure 1e-4 of |norm| + |mu|"""
    from bioem_amd import engine as eng
    from bioem_amd import soft_views as sv
    S = oracle_setup(load_case(name))
    pmap, _ = S.run(1)
    worst = 0.0
    for p in range(min(S.nMaps, 4)):
        r = pmap[p]
        conv, p5 = S.conv_spectra(int(r["orient"]))
        c = int(r["conv"])
        Smap, _ = wr.s_map(conv[c], S.refFFT[p])
        cc = wr.cc_of(Smap[(-int(r["cent_x"])) % S.N, (-int(r["cent_y"])) % S.N], S.N)
        par = np.zeros(1, dtype=eng.PARAM5_DTYPE)
        par[0] = tuple(p5[c])
        norm, mu = sv.cell_params(np.full((1, 1, 1), cc, dtype=np.float32), par, S.sumRef[p:p + 1], S.N)
        d = max(abs(norm[0, 0, 0] - float(r["norm"])), abs(mu[0, 0, 0] - float(r["mu"])))
        worst = max(worst, d / (abs(float(r["norm"])) + abs(float(r["mu"]))))
    print("cell_params %s: worst difference %.3g of |norm| + |mu| (figure 1e-4)" % (name, worst))
    assert worst <= 1e-4


def test_members_masses_add_up_and_weights_scale():
    from bioem_amd import soft_views as sv
    nd, N = 5, 16
    req, logp, cc, par = planted(7, nd, 2)
    req["particle"] = [0, 0, 0, 2, 2, 3, 3]
    req["orient"] = [4, 4, 1, 0, 0, 2, 5]
    req["conv"] = [0, 1, 0, 0, 1, 1, 1]
    group = req["orient"].astype(np.int32)
    sums = np.array([1.0, 0.0, -3.0, 2.0], dtype=np.float32)
    m, cells, w = sv.members(req, group, logp, cc, par, sums, N, want_weights=True)
    assert m.dtype.itemsize == 40 and cells.shape == (7, nd, nd) and np.array_equal(m["group"], group)
    for p in (0, 2, 3):
        sel = req["particle"] == p
        assert abs(m["mass"][sel].sum() - 1.0) <= 4 * sr.U * sel.sum() * nd * nd
        # the weights are the softmax of logp over all cells of the particle's requests
        t = logp[sel]
        want = np.exp(t - wr.lse(t))
        assert np.allclose(w[sel], want, rtol=1e-12, atol=0)
    norm, mu = sv.cell_params(cc, par, sums[req["particle"]], N)
    assert np.allclose(cells, w * norm, rtol=1e-15) and np.allclose(m["s2"], (w * norm * norm).sum(axis=(1, 2)), rtol=1e-14)
    assert np.allclose(m["b"], (w * norm * mu).sum(axis=(1, 2)), rtol=1e-12, atol=1e-15)
    # weights multiply a, s2, b and mass; a zero weight keeps the member with an empty table
    W = np.array([2.0, 9.0, 0.0, 0.5])
    m2, cells2 = sv.members(req, group, logp, cc, par, sums, N, weights=W)
    f = W[req["particle"]]
    assert np.array_equal(cells2, f[:, None, None] * cells)
    for k in ("s2", "b", "mass"):
        assert np.array_equal(m2[k], f * m[k]), k
    # a log prior per orientation moves mass between a particle's orientations, not between particles
    prior = np.array([0.0, -2.0, 0.0, 0.0, 1.0, -1.0])
    m3, _, w3 = sv.members(req, group, logp, cc, par, sums, N, log_prior=prior, want_weights=True)
    t = logp[:3] + prior[req["orient"][:3]][:, None, None]
    assert np.allclose(w3[:3], np.exp(t - wr.lse(t)), rtol=1e-12, atol=0)
    assert abs(m3["mass"][:3].sum() - 1.0) <= 1e-14 and np.allclose(w3[3:5], w[3:5], rtol=1e-13, atol=0)
    s = sv.particle_summary(req, w, 4)
    assert s["requests"].tolist() == [3, 0, 2, 2] and s["n_eff"][1] == 0.0 and (s["n_eff"][[0, 2, 3]] > 1.0).all()
    assert np.array_equal(s["mass_argmax"], [w[:3].max(), 0.0, w[3:5].max(), w[5:].max()])


def test_members_one_hot_limit_and_non_finite_cells():
    from bioem_amd import soft_views as sv
    nd, N = 3, 16
    req, logp, cc, par = planted(4, nd, 3)
    req["particle"] = [0, 0, 1, 2]
    req["conv"] = [0, 1, 0, 0]
    group = np.array([5, 5, 6, 7], dtype=np.int32)
    sums = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    # a planted peak 800 above the rest: every other cell underflows to weight 0 exactly
    logp[:2] = -1000.0
    logp[1, 2, 0] = -200.0
    # particle 1: NaN, +inf and -inf cells are left out, the rest is normalised; particle 2: nothing finite
    logp[2, 0, 0], logp[2, 0, 1], logp[2, 1, 1] = np.nan, np.inf, -np.inf
    logp[3] = np.nan
    m, cells, w = sv.members(req, group, logp, cc, par, sums, N, want_weights=True)
    norm, mu = sv.cell_params(cc, par, sums[req["particle"]], N)
    assert w[1, 2, 0] == 1.0 and w[:2].sum() == 1.0 and not cells[0].any() and m["mass"][0] == 0.0
    assert np.count_nonzero(cells[1]) == 1 and cells[1, 2, 0] == norm[1, 2, 0]
    assert m["s2"][1] == norm[1, 2, 0] ** 2 and m["b"][1] == norm[1, 2, 0] * mu[1, 2, 0] and m["mass"][1] == 1.0
    assert m["group"].tolist() == [5, 5, 6, -1]
    assert w[2, 0, 0] == 0.0 and w[2, 0, 1] == 0.0 and w[2, 1, 1] == 0.0 and abs(w[2].sum() - 1.0) <= 1e-15
    assert np.isfinite(cells).all() and not cells[3].any() and m["mass"][3] == 0.0 and m["s2"][3] == 0.0
    for k in ("s2", "b", "mass"):
        assert np.isfinite(m[k]).all()


def test_requests_best_and_topk():
    from bioem_amd import engine as eng
    from bioem_amd import soft_views as sv
    raw, pmap, _ = eng.new_prob_block(4, 9, 0)
    pmap["Total"][[0, 1, 3]] = 1.0
    pmap["Constoadd"][[0, 1, 3]] = -5.0
    pmap["orient"] = [7, 2, 0, -1]
    req, group = sv.requests_best(pmap, 3)
    assert req["particle"].tolist() == [0, 0, 0, 1, 1, 1] and req["orient"].tolist() == [7, 7, 7, 2, 2, 2]
    assert req["conv"].tolist() == [0, 1, 2, 0, 1, 2] and group.tolist() == req["orient"].tolist() and group.dtype == np.int32
    cand = np.zeros((3, 3), dtype=eng.CANDIDATE_DTYPE)
    cand["orient"] = [[4, 1, 8], [2, -1, -1], [0, 5, 3]]
    req, group = sv.requests_topk(cand, 2, 2)
    assert req["particle"].tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2, 2]
    assert req["orient"].tolist() == [4, 4, 1, 1, 2, 2, 0, 0, 5, 5] and req["conv"].tolist() == [0, 1] * 5
    assert group.tolist() == req["orient"].tolist()
    one, _ = sv.requests_topk(cand, 1, 1)
    assert one["orient"].tolist() == [4, 2, 0]
    with pytest.raises(ValueError):
        sv.requests_topk(cand, 4, 2)


def test_text_lines_round_trip(tmp_path):
    from bioem_amd import reconstruct as rc
    from bioem_amd import soft_views as sv
    rng = np.random.default_rng(4)
    N = 8
    A, B = np.fft.rfftn(rng.standard_normal((N, N, N))), np.fft.rfftn(rng.standard_normal((N, N, N)))
    hard, soft = rc.shell_sums(A, B), rc.shell_sums(A, A + 0.25 * B)
    path = str(tmp_path / "recon.txt")
    rc.write(path, hard, N, 1.5, 7, 123, 0.03125)
    before = open(path).read()
    summary = np.zeros(3, dtype=sv.PARTICLE_DTYPE)
    summary["particle"], summary["requests"] = np.arange(3), [4, 0, 8]
    summary["n_eff"], summary["mass_argmax"] = [1.25, 0.0, 17.5], [0.875, 0.0, 0.0625]
    sv.write(path, summary, soft, N, 1.5)
    assert open(path).read().startswith(before)
    got, shells = sv.parse(path)
    assert got.tobytes() == summary.tobytes()
    f, res, _, _ = rc.derive(soft[1], soft[2], soft[3], N, 1.5)
    assert np.array_equal(shells["weight"], soft[0]) and np.array_equal(shells["FSC"], np.array([float("%.15e" % x) for x in f]))
    assert np.array_equal(shells["cross"], np.array([float("%.15e" % x) for x in soft[1]]))
    # the hard lines still parse beside them
    hs, data = rc.parse(path)
    assert np.array_equal(hs["weight"], hard[0]) and int(data["particles"]) == 123
    with open(path, "a") as f2:
        f2.write("SOFT 3 1\n")
    with pytest.raises(ValueError):
        sv.parse(path)


def test_cli_refusals_that_need_no_device(tmp_path):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"

    def run(args):
        return subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              timeout=60)
    r = run(["--PrintBestCalMap", "best.txt", "--Modelfile", "m.txt", "--Reconstruct", "recon", "--ReconstructSoft", "1"])
    assert r.returncode == 1 and "--PrintBestCalMap goes without" in r.stdout
    text = ("NUMBER_PIXELS 32\nPIXEL_SIZE 1.77\nCTF_DEFOCUS 2.0 2.0 1\nCTF_B_ENV 2.0 2.0 1\nCTF_AMPLITUDE 0.1 0.1 1\n"
            "DISPLACE_CENTER 2 1\nUSE_QUATERNIONS\nGRIDPOINTS_QUATERNION 2\n")
    (tmp_path / "param.txt").write_text(text)
    (tmp_path / "angles1.txt").write_text(text + "WRITE_PROB_ANGLES 1\n")
    (tmp_path / "grid.txt").write_text("1\n 0.00000000  0.00000000  0.00000000  1.00000000 \n")
    base = ["--Modelfile", "none.txt", "--Particlesfile", "none.txt", "--Inputfile"]
    r = run(base + ["param.txt", "--ReconstructSoft", "1"])
    assert r.returncode == 1 and "--ReconstructSoft goes with --Reconstruct" in r.stdout
    for bad in ("0", "-2", "x"):
        r = run(base + ["param.txt", "--Reconstruct", "recon", "--ReconstructSoft", bad])
        assert r.returncode == 1 and "--ReconstructSoft needs a positive number of orientations" in r.stdout, bad
    for param, K in (("param.txt", "2"), ("angles1.txt", "2"), ("angles1.txt", "3")):
        r = run(base + [param, "--Reconstruct", "recon", "--ReconstructSoft", K])
        assert r.returncode == 1 and "--ReconstructSoft %s needs WRITE_PROB_ANGLES %s or more" % (K, K) in r.stdout, (param, K)
    # whatever --Reconstruct is refused with
    r = run(base + ["param.txt", "--Reconstruct", "recon", "--ReconstructSoft", "1", "--RefineOrientations", "grid.txt"])
    assert r.returncode == 1 and "--Reconstruct is not valid with --RefineOrientations" in r.stdout
    r = run(base + ["param.txt", "--Reconstruct", "recon", "--ReconstructSoft", "1", "--ReconstructWiener", "-1"])
    assert r.returncode == 1 and "--ReconstructWiener needs a non-negative number" in r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["angles1.txt", "grid.txt", "param.txt"]
    r = run(["--help"])
    assert "--ReconstructSoft arg" in r.stdout and "WRITE_PROB_ANGLES >= arg" in r.stdout
