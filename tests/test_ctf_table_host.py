"""The posterior per CTF set and particle, host side (no device): the two ABI entries, the --ProbCTF writer through
hostlib and its parser (bioem_amd/ctf_prob.py), and the merge of shard tables over bioem_hip_merge_host."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_PROB = -999999.0


def test_header_library_and_exports_name_the_two_entries():
    import bioem_amd.engine as eng
    hdr = open(os.path.join(ROOT, "include", "bioem_hip.h")).read()
    assert re.search(r"^int bioem_hip_enable_ctf_table\(bioem_hip_handle h, int on\);", hdr, re.M)
    assert re.search(r"^int bioem_hip_ctf_table\(bioem_hip_handle h, bioem_hip_prob_map \*out\);", hdr, re.M)
    assert "bioem_hip_merge_host(nShards, nCTF * nMaps, 0, 0, tables, out)" in hdr     # how shards are merged
    L = eng.load_library()
    for name in ("bioem_hip_enable_ctf_table", "bioem_hip_ctf_table"):
        assert hasattr(L, name) and name in eng.EXPORTS
    assert callable(eng.Engine.enable_ctf_table) and callable(eng.Engine.ctf_table) and callable(eng.merge_ctf_tables)


def synthetic_table():
    """[3 CTF sets][2 particles] with known values"""
    import bioem_amd.engine as eng
    t = np.zeros((3, 2), dtype=eng.PROB_MAP_DTYPE)
    t["Total"] = [[1.0, 2.5], [3.25, 1.0e-3], [7.0, 1.5]]
    t["Constoadd"] = [[-77000.125, -76990.5], [-77010.0625, -76000.25], [-76999.5, -77777.75]]
    t["orient"] = [[0, 3], [1, 2], [3, 0]]
    t["conv"] = [[0, 0], [1, 1], [2, 2]]
    t["cent_x"] = [[-3, 4], [0, 10], [-10, 1]]
    t["cent_y"] = [[2, -1], [7, 0], [5, -6]]
    t["norm"] = [[0.5, 1.25], [2.0625, 0.03125], [10.5, 0.75]]
    t["mu"] = [[-0.25, 0.0], [0.125, -1.5], [3.0, 0.0625]]
    return t


ANGLES = np.array([[0.1, 0.2, 0.3, 0.9273618], [-0.5, 0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 1.0], [0.70710678, 0.0, -0.70710678, 0.0]],
                  dtype=np.float32)
CTF_PARAM = np.array([[0.1, 1500.0, 2.0], [0.1, 3000.0, 151.0], [0.25, 4100.0, 300.0]], dtype=np.float32)
ELECWAVEL = np.float32(0.019688)
NTOTPI, VOLU = np.float32(64 * 64), np.float32(3.2e-7)


def f4(x):
    return "%.4f" % float(x)


@pytest.mark.parametrize("quat", [True, False])
@pytest.mark.parametrize("psf", [False, True])
def test_writer_and_parser_round_trip(quat, psf, tmp_path):
    from bioem_amd import ctf_prob, hostlib
    t = synthetic_table()
    path = str(tmp_path / "CTF_PROB")
    hostlib.write_ctf_prob(path, t, CTF_PARAM, ANGLES, NTOTPI, VOLU, usepsf=psf, elecwavel=ELECWAVEL, isQuat=quat)
    text = open(path).read()
    lines = text.split("\n")
    assert lines[0] == ctf_prob.BAR and lines[2] == ctf_prob.BAR and lines[-1] == ""
    assert ("PSF amp" in lines[1]) == psf and ("q4" in lines[1]) == quat
    body = lines[3:-1]
    assert len(body) == 6
    # the layout, line by line, restated here: particle-major, fixed, 4 decimals
    numconst = 0.5 * math.log(math.pi) + (1.0 - float(NTOTPI) * 0.5) * (math.log(2.0 * math.pi) + 1.0) + math.log(float(VOLU))
    nA = 4 if quat else 3
    for n, ln in enumerate(body):
        i, c = divmod(n, 3)
        e = t[c, i]
        k = CTF_PARAM[c]
        k1 = float(k[1]) if psf else float(np.float32(k[1]) / np.float32(2.0)) / math.pi / float(ELECWAVEL) * 0.0001
        logp = math.log(e["Total"]) + e["Constoadd"] + numconst
        want = " %d %d %s %s %s %s Separated: %s %s %s Best: %s %d %d %s %s" % (
            i, c, f4(k[0]), f4(k1), f4(k[2]), f4(logp), f4(math.log(e["Total"])), f4(e["Constoadd"]), f4(numconst),
            " ".join(f4(v) for v in ANGLES[e["orient"]][:nA]), e["cent_x"], e["cent_y"], f4(e["norm"]), f4(e["mu"]))
        assert ln == want
        assert all(re.fullmatch(r"-?\d+\.\d{4}", tok) for tok in ln.split()[2:6])
    if not psf:        # the defocus column is in micro-m: phase / (2 pi lambda 1e4)
        assert [ln.split()[3] for ln in body[:3]] == [f4(v) for v in CTF_PARAM[:, 1].astype(np.float64) / (2 * math.pi * float(ELECWAVEL) * 1e4)]
    rows, notation = ctf_prob.parse(path)
    assert notation == lines[1] and rows.shape == (2, 3) and rows["A"].shape == (2, 3, nA)
    want = ctf_prob.rows_from_table(t, CTF_PARAM, ANGLES, NTOTPI, VOLU, usepsf=psf, elecwavel=ELECWAVEL, isQuat=quat)
    for f in ("particle", "ctf", "cent_x", "cent_y"):
        assert np.array_equal(rows[f], want[f])
    for f in ("k", "logP", "logTotal", "Constoadd", "numconst", "A", "norm", "mu"):
        assert np.abs(rows[f] - want[f]).max() <= 0.5001e-4, f
    # logP against numpy, and the lines of a particle sum to what its LogProb line would carry
    lt = np.log(t["Total"]) + t["Constoadd"]
    assert np.abs(rows["logP"] - (lt.T + numconst)).max() <= 0.5001e-4
    m = lt.max(axis=0)
    whole = m + np.log(np.exp(lt - m).sum(axis=0)) + numconst
    assert np.abs(ctf_prob.particle_logp(rows) - whole).max() <= 2e-4


def test_writer_with_a_list_and_a_volume_element_per_map(tmp_path):
    """round 2: angles_per_map entries per particle, volu per map in numconst and logP"""
    from bioem_amd import ctf_prob, hostlib
    t = synthetic_table()
    t["orient"] = [[0, 1], [1, 0], [1, 1]]
    vol = np.array([3.2e-7, 1.1e-6], dtype=np.float32)
    path = str(tmp_path / "CTF_PROB_Round2")
    hostlib.write_ctf_prob(path, t, CTF_PARAM, ANGLES, NTOTPI, VOLU, elecwavel=ELECWAVEL, angles_per_map=2, volu_per_map=vol)
    rows, _ = ctf_prob.parse(path)
    want = ctf_prob.rows_from_table(t, CTF_PARAM, ANGLES, NTOTPI, vol, elecwavel=ELECWAVEL, angles_per_map=2)
    assert np.abs(rows["A"][1, 0] - ANGLES[2 + 1]).max() <= 0.5001e-4       # particle 1, CTF 0: entry 1 of ITS list
    assert np.abs(rows["A"] - want["A"]).max() <= 0.5001e-4
    nc = 0.5 * math.log(math.pi) + (1.0 - float(NTOTPI) * 0.5) * (math.log(2.0 * math.pi) + 1.0) + np.log(vol.astype(np.float64))
    assert np.abs(rows["numconst"] - nc[:, None]).max() <= 0.5001e-4
    assert np.abs(rows["logP"] - want["logP"]).max() <= 0.5001e-4


def test_writer_refuses_an_untouched_entry(tmp_path):
    from bioem_amd import hostlib
    t = synthetic_table()
    t[2, 1] = np.zeros((), dtype=t.dtype)
    t[2, 1]["Constoadd"] = MIN_PROB           # as start_run leaves it
    path = str(tmp_path / "CTF_PROB")
    with pytest.raises(ValueError, match=r"RefMap 1 .*CTF set 2"):
        hostlib.write_ctf_prob(path, t, CTF_PARAM, ANGLES, NTOTPI, VOLU, elecwavel=ELECWAVEL)
    assert not os.path.exists(path)


def test_parser_refuses_other_files(tmp_path):
    from bioem_amd import ctf_prob
    p = tmp_path / "x"
    p.write_text("RefMap: 0 LogProb:  -1.0 Constant: -2.0\n")
    with pytest.raises(ValueError, match="HEADER"):
        ctf_prob.parse(str(p))
    p.write_text(ctf_prob.BAR + "\nnotation\n" + ctf_prob.BAR + "\n 0 0 1.0 2.0\n")
    with pytest.raises(ValueError, match="malformed"):
        ctf_prob.parse(str(p))


def test_merge_ctf_tables_is_the_entry_rule_and_ties_go_to_the_first_table():
    import bioem_amd.engine as eng
    rng = np.random.default_rng(11)
    tabs = []
    for s in range(2):
        t = np.zeros((3, 4), dtype=eng.PROB_MAP_DTYPE)
        t["Total"] = rng.uniform(0.5, 40.0, size=t.shape)
        t["Constoadd"] = -77000.0 + np.round(rng.uniform(-30.0, 30.0, size=t.shape), 3)
        for f in ("orient", "conv", "cent_x", "cent_y"):
            t[f] = rng.integers(-9, 90, size=t.shape)
        t["norm"] = rng.uniform(0.1, 3.0, size=t.shape)
        t["mu"] = rng.uniform(-1.0, 1.0, size=t.shape)
        tabs.append(t)
    tabs[1]["Constoadd"][1, 2] = tabs[0]["Constoadd"][1, 2]      # a tie: the record of the FIRST table
    tabs[1][0, 3] = np.zeros((), dtype=tabs[1].dtype)            # an entry the second shard never touched
    tabs[1]["Constoadd"][0, 3] = MIN_PROB
    tabs[0][2, 0] = tabs[1][0, 3]                                # and one the first never touched
    got = eng.merge_ctf_tables(tabs)
    assert got.shape == (3, 4) and got.dtype == eng.PROB_MAP_DTYPE
    a, b = tabs
    first = a["Constoadd"] >= b["Constoadd"]
    cmax = np.maximum(a["Constoadd"], b["Constoadd"])
    total = a["Total"] * np.exp(a["Constoadd"] - cmax) + b["Total"] * np.exp(b["Constoadd"] - cmax)
    assert np.array_equal(got["Constoadd"], cmax)
    assert np.abs(got["Total"] - total).max() <= 4 * np.finfo(np.float64).eps * np.abs(total).max()
    for f in ("orient", "conv", "cent_x", "cent_y", "norm", "mu"):
        assert np.array_equal(got[f], np.where(first, a[f], b[f])), f
    assert first[1, 2] and got[1, 2]["orient"] == a[1, 2]["orient"]
    assert got[0, 3].tobytes() == a[0, 3].tobytes() and got[2, 0].tobytes() == b[2, 0].tobytes()
