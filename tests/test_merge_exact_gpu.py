"""The device's half of the merge of shards against tests/merge_reference.py: k_topk_angles (list widths K and 2K - 1) and
k_merge_shards with more than one shard, through the hooks bioem_hip_debug_topk and bioem_hip_debug_merge_gathered (the
half of bioem_hip_merge behind its all-gather; no RCCL, one GPU).  tests/test_merge_reference_host.py runs the same
cases through the host's half.

a  k_topk_angles on tables handed in: all 3^8 key patterns over {-inf, 0, 1} as the 6 561 particles of one launch (keys
   exact: forAngles = 1, integer ConstAngle and numconst), K = 1 ... 4, W = K and 2K - 1, every slot and every field
   against merge_reference.shard_list; nMaps 1, 63, 64, 65 (the 64-thread block); o0 > 0, nO < K, nO = K, K = 1.
b  the same tables cut into two shards (every cut) and three (a seeded selection): debug_topk per shard, then the wide
   merge, must be writer_heap of the whole table.
c  k_merge_shards: the map-entry cases of the host test with nMaps 1, 127, 128, 129, 300 (the 128-thread block), 1, 2, 3
   and 8 shards, K = 0 and K = 5 (the two payload strides); every payload carries its shard's candidate list, unused
   slots filled with 0xff bytes (orient -1 and NaN: a wrong offset or stride shows).  The host test's assertions, and
   bit for bit bioem_hip_merge_host's Constoadd and records and bioem_hip_merge_topk_host_wide's candidates.
d  real runs: lists of three orientations only (the particles' own twice, two others ten and more times, interleaved),
   so that the K-th key of every particle is a tie; three shard handles cut inside the runs of equal keys; the wide
   merge of merge_candidates equals the unsharded handle's topk_angles in every field; the reference's K-wide merge of
   the same table does not (asserted, or the test tests nothing).  The CLI on the g11 Euler list with repeated rows
   (every copy its own prior, which the file prints), 1 and 3 shards, against the oracle's ang_prob_rows.

B (merge_reference.bound) is derived from the operations, not tuned.  Largest |d log P| / B as measured on an MI355X
(every test of c prints its own): 0.226 at every particle count, reached with three shards; per shard count the device
gives what the host gives (tests/test_merge_reference_host.py: 0.000 with one shard, 0.103 with 2, 0.226 with 3, 0.128
with 8).  No failing entry, slot or field in a, b, c or d.

Strength (one scratch copy of the library per slip, none committed, every index in range; the CLI cases run the
installed library and do not see a scratch one):
  `>=` for `>` in k_merge_shards                     fails c: all four particle counts and the one-particle test
  the stride taken as mapBytes when K > 0            fails c: the same five
  `<=` for `<` in the replacement of k_topk_angles   fails every a and b test, d (shard handles), test_g_topk_with_equal_keys
  the second walk dropped                            fails a (K >= 2, particle counts, short blocks), b (K >= 2),
                                                     d (shard handles)
  minIo ignored in cand_less                         fails a (K >= 2, particle counts, short blocks), d (shard handles),
                                                     test_g_topk_with_equal_keys of tests/test_fold_exact.py

"""
import os
import random
import subprocess

import numpy as np
import pytest

import merge_cases as mc
from merge_reference import merge_lists, shard_list, writer_heap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def bare_engine(nMaps):
    """a handle of nMaps particles with nothing uploaded: the hooks run on what is handed in"""
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
    from bioem_amd.synthetic import ELECWAVEL, make_param_device
    import math
    fac = math.pi * 2.0 * 10000 * float(ELECWAVEL)
    px = np.float32(1.77)
    _, _, steps = hostlib.ctf_kernels(32, px, (np.float32(0.1), np.float32(0.1), 1), (np.float32(fac), np.float32(4.0 * fac), 1),
                                      (np.float32(2.0), np.float32(300.0), 1))
    pd = make_param_device(32, 3, 1, 8, steps, 1, px)
    return eng.Engine(pd, nMaps, 8, 1, algo=1, device=0)


@pytest.fixture(scope="module")
def hook():
    E = bare_engine(1)
    yield E
    E.close()


@pytest.fixture(scope="module")
def exhaustive():
    pats = mc.exhaustive_patterns()
    return pats, mc.pack_table(pats)


# ------------------------------------------------------------------------------------------------------
# a. k_topk_angles on tables handed in
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_a_every_pattern_every_slot(hook, exhaustive, K):
    pats, tab = exhaustive
    first = None
    for W in sorted({K, 2 * K - 1}):
        got = hook.debug_topk(tab, 0, K, W, mc.NUMCONST)
        want = mc.SegmentLists(pats, K, W).block(0, 8)
        bad = [p for p in range(len(pats)) if not same(got[p], want[p])]
        assert not bad, (K, W, len(bad), pats[bad[0]], got[bad[0]], want[bad[0]])
        if first is None:
            first = got
        assert same(got[:, :K], first[:, :K])                   # slots 0 ... K-1 do not depend on the width
        assert same(hook.debug_topk(tab, 0, K, W, mc.NUMCONST), got)


@pytest.mark.parametrize("nMaps", [1, 63, 64, 65])
def test_a_particle_counts_around_the_block(hook, exhaustive, nMaps):
    pats, _ = exhaustive
    rng = random.Random(20261025 + nMaps)
    pick = rng.sample(pats, nMaps)
    tab = mc.pack_table(pick)
    for K in (1, 2, 3, 4):
        for W in sorted({K, 2 * K - 1}):
            assert same(hook.debug_topk(tab, 0, K, W, mc.NUMCONST), mc.SegmentLists(pick, K, W).block(0, 8)), (K, W)


def test_a_offsets_and_short_blocks(hook, exhaustive):
    pats, tab = exhaustive
    for K in (1, 2, 3, 4):
        for W in sorted({K, 2 * K - 1}):
            seg = mc.SegmentLists(pats, K, W)
            for a, b in [(0, 1), (0, K), (8 - K, 8), (3, 8), (5, 6), (2, 2 + max(1, K - 1)), (1, 8)]:
                got = hook.debug_topk(np.ascontiguousarray(tab[a:b]), a, K, W, mc.NUMCONST)
                assert same(got, seg.block(a, b)), (K, W, a, b)
            # the global index is o0 + row: the same rows further up the list
            got = hook.debug_topk(np.ascontiguousarray(tab[3:8]), 1000003, K, W, mc.NUMCONST)
            want = seg.block(3, 8)
            want["orient"] = np.where(want["orient"] >= 0, want["orient"] + 1000000, -1)
            assert same(got, want)


def test_a_refusals(hook, exhaustive):
    _, tab = exhaustive
    for K, W in [(0, 0), (3, 4), (3, 6), (2, 1)]:
        with pytest.raises(RuntimeError) as e:
            hook.debug_topk(tab[:, :4], 0, K, W, mc.NUMCONST)
        assert e.value.rc == 2
    with pytest.raises(RuntimeError) as e:
        hook.debug_topk(tab[:, :4], -1, 2, 3, mc.NUMCONST)
    assert e.value.rc == 2
    assert hook.debug_topk(tab[:, :4], 0, 2, 3, mc.NUMCONST).shape == (4, 3)        # the handle is still usable


# ------------------------------------------------------------------------------------------------------
# b. sharded, on the same tables
# ------------------------------------------------------------------------------------------------------
def device_list(hook, tab, a, b, K, W):
    import bioem_amd.engine as eng
    if a == b:                                                   # a shard that owns nothing offers nothing
        out = np.zeros((tab.shape[1], W), dtype=eng.CANDIDATE_DTYPE)
        out[:] = mc.pack_list([None] * W, W)
        return out
    return hook.debug_topk(np.ascontiguousarray(tab[a:b]), a, K, W, mc.NUMCONST)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_b_shards_of_the_device_merge_to_the_writers_walk(hook, exhaustive, K):
    import bioem_amd.engine as eng
    pats, tab = exhaustive
    W = 2 * K - 1
    want = mc.expected_topk(pats, K)
    rng = random.Random(20261026 + K)
    three = mc.cuts(8, 3)
    chosen = mc.cuts(8, 2) + rng.sample(three, 12)
    cache = {}
    narrow_wrong = 0
    for cut in chosen:
        lists = []
        for a, b in zip(cut, cut[1:]):
            if (a, b) not in cache:
                cache[(a, b)] = device_list(hook, tab, a, b, K, W)
            lists.append(cache[(a, b)])
        got = eng.merge_topk_host(lists, K)
        bad = [p for p in range(len(pats)) if not same(got[p], want[p])]
        assert not bad, (K, cut, len(bad), pats[bad[0]], got[bad[0]], want[bad[0]])
        narrow = eng.merge_topk_host([np.ascontiguousarray(x[:, :K]) for x in lists])
        narrow_wrong += not same(narrow, want)
    assert (narrow_wrong > 0) == (K > 1)                         # the device's K-wide lists are not enough either


# ------------------------------------------------------------------------------------------------------
# c. k_merge_shards and the candidate offsets, through the half of bioem_hip_merge behind the all-gather
# ------------------------------------------------------------------------------------------------------
MERGE_K = 5


def gathered_payloads(blocks, lists):
    """what the all-gather leaves: per shard its map entries, then (lists given) its nMaps candidate lists; unused
    candidate slots are 0xff bytes throughout"""
    S = blocks.shape[0]
    parts = []
    for s in range(S):
        parts.append(np.ascontiguousarray(blocks[s]).view(np.uint8).reshape(-1))
        if lists is not None:
            raw = np.ascontiguousarray(lists[s]).copy()
            flat = raw.view(np.uint8).reshape(-1, raw.dtype.itemsize)
            flat[raw.reshape(-1)["orient"] < 0] = 0xff
            parts.append(flat.reshape(-1))
    return np.concatenate(parts)


def candidate_inputs(n, S, seed):
    rng = random.Random(seed)
    tables = mc.random_tables(count=n, nO=14, seed=seed, values=(mc.NINF, 0.0, 1.0, 2.0))
    cutsets = [mc.random_cut(rng, 14, S) for _ in range(n)]
    W = 2 * MERGE_K - 1
    lists = [np.stack([mc.pack_list(shard_list(t[c[s]:c[s + 1]], c[s], MERGE_K, W), W) for t, c in zip(tables, cutsets)])
             for s in range(S)]
    return tables, lists


def run_gathered(E, cases, S, K, first, worst):
    import bioem_amd.engine as eng
    n = E.nMaps
    blocks = mc.pack_maps(cases, S, n=n, first=first)
    tables, lists = candidate_inputs(n, S, 20261027 + 31 * S + n + first) if K else (None, None)
    pmap, cand = E.debug_merge_gathered(gathered_payloads(blocks, lists), S, K)
    worst[0] = max(worst[0], mc.check_maps(pmap, blocks, cases, first=first))
    host = eng.merge_host([np.ascontiguousarray(blocks[s]).view(np.uint8).reshape(-1) for s in range(S)], n, 0, 0)
    host = host.view(eng.PROB_MAP_DTYPE)
    for f in ("Constoadd",) + mc.RECORD:
        assert same(pmap[f], host[f]), (S, K, n, f)
    if K:
        assert same(cand, eng.merge_topk_host(lists, K))
        assert same(cand, mc.expected_topk(tables, K))
    else:
        assert cand is None


@pytest.mark.parametrize("nMaps", [127, 128, 129, 300])
def test_c_merge_of_gathered_shards(nMaps):
    E = bare_engine(nMaps)
    worst = [0.0]
    for S in (1, 2, 3, 8):
        cases = mc.map_cases(S)
        assert len(cases) <= nMaps                               # every case is an entry of the block
        for K in (0, MERGE_K):
            run_gathered(E, cases, S, K, 3 * S + K, worst)
    E.close()
    print("k_merge_shards, %d particles: largest |d log P| / B = %.3f" % (nMaps, worst[0]))


def test_c_merge_of_gathered_shards_one_particle(hook):
    worst = [0.0]
    for S in (1, 2, 3, 8):
        cases = mc.map_cases(S)
        for i in range(len(cases)):
            run_gathered(hook, cases, S, MERGE_K if i % 2 else 0, i, worst)
    print("k_merge_shards, one particle: largest |d log P| / B = %.3f" % worst[0])


def test_c_refusals(hook):
    cases = mc.map_cases(2)
    blocks = mc.pack_maps(cases, 2, n=1)
    good = gathered_payloads(blocks, None)
    pm = np.zeros(1, dtype=blocks.dtype)
    for nShards, K in [(0, 0), (2, -1), (2, 3)]:                 # K > 0 without a place for the candidates
        assert hook.L.bioem_hip_debug_merge_gathered(hook.h, good.ctypes.data, nShards, K, pm.ctypes.data, None) == 2
    assert hook.L.bioem_hip_debug_merge_gathered(hook.h, None, 2, 0, pm.ctypes.data, None) == 2
    pmap, _ = hook.debug_merge_gathered(good, 2, 0)              # the handle is still usable
    mc.check_maps(pmap, blocks, cases)


# ------------------------------------------------------------------------------------------------------
# d. real runs
# ------------------------------------------------------------------------------------------------------
LAYOUT = "ABAB" + "ABABABABABoAB" + "BABABAoBA"           # o: the particles' own orientation; cuts after 4 and 17
CUTS = (0, 4, 17, len(LAYOUT))
REAL_K = 5


def test_d_three_shard_handles_cut_inside_runs_of_equal_keys():
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
    from bioem_amd.synthetic import random_quaternions, synth_model
    from test_fold_exact import PX, TIE_SNR, Rig
    K, T, numconst, nP = REAL_K, len(LAYOUT), -1234.5, 5
    pool = random_quaternions(8, seed=20260777)
    quats = np.stack([pool[{"o": 0, "A": 1, "B": 2}[c]] for c in LAYOUT])
    # the table itself, from a plain handle: equal rows give equal keys whatever forms them
    plain = Rig(nP, T, 1, quats=quats)
    plain.render(TIE_SNR, truth=[(LAYOUT.index("o"), 0)] * nP)
    pang = plain.run(lambda e: e.project_convolve_compare(0, T))[1][:T]
    plain.close()
    refs = []
    for p in range(nP):
        keys = [float(k) for k in np.log(pang["forAngles"][:, p]) + pang["ConstAngle"][:, p] + numconst]
        ref = writer_heap(keys, K)
        t = ref[-1][0]
        assert sum(1 for k in keys if k == t) > sum(1 for k, _ in ref if k == t), ("no tie at the K-th key", p)
        assert [LAYOUT[o] for _, o in ref[:2]] == ["o", "o"] and len({LAYOUT[o] for _, o in ref[2:]}) == 1, (p, ref)
        narrow = merge_lists([shard_list(keys[a:b], a, K, K) for a, b in zip(CUTS, CUTS[1:])], K)
        assert narrow != ref, ("the cuts do not matter for this particle", p)
        wide = merge_lists([shard_list(keys[a:b], a, K, 2 * K - 1) for a, b in zip(CUTS, CUTS[1:])], K)
        assert wide == ref
        refs.append(ref)
    # the unsharded handle
    whole = Rig(nP, T, 1, shard=True, quats=quats)
    whole.render(None, maps=plain.maps)
    whole.run(lambda e: e.project_convolve_compare(0, T))
    want = whole.E.topk_angles(K, numconst)
    assert same(whole.E.merge_candidates(K, numconst)[:, :K], want)
    for p in range(nP):
        assert [o for _, o in refs[p]] == [int(o) for o in want[p]["orient"]], p
        for c in want[p]:
            assert same(c["forAngles"], pang["forAngles"][c["orient"], p])
            assert same(c["ConstAngle"], pang["ConstAngle"][c["orient"], p])
    # three shard handles on the one GPU
    points, NormDen = hostlib.center_model(synth_model(40, 8.0, 18.0))
    lists = []
    for a, b in zip(CUTS, CUTS[1:]):
        E = eng.Engine(whole.pd, nP, T, 1, algo=1, device=0, shard=(a, b))
        E.upload_ctf(whole.refCTF, whole.ctfParam)
        E.upload_model(points, NormDen, np.float32(PX))
        E.upload_orientations(quats, True)
        E.upload_particle_maps(plain.maps)
        raw, _, _ = eng.new_prob_block(nP, 0, 0)
        E.start_run(raw)
        E.project_convolve_compare(a, b)
        E.finish_run(raw)
        lists.append(E.merge_candidates(K, numconst))
        assert same(lists[-1][:, :K], E.topk_angles(K, numconst))
        E.close()
    whole.close()
    got = eng.merge_topk_host(lists, K)
    assert same(got, want), (got["orient"], want["orient"])
    narrow = eng.merge_topk_host([np.ascontiguousarray(x[:, :K]) for x in lists])
    assert not np.any(np.all(narrow["orient"] == want["orient"], axis=1))        # the K-wide merge: wrong for every particle


def g11_with_repeated_rows():
    """the g11 case on a list of 42 rows, three blocks of 14: the particles' best rows H once in the second and once in
    the third block, their common second-best row M twice in the first block, four times at the head of the second (before
    H) and twice in the third; the other rows fill up.  Every copy carries its own prior, which ANG_PROB prints."""
    from golden_util import load_case
    import oracle as orc
    case = load_case("g11_n32_eulerlist")
    S0 = orc.Setup(case["P"], case["model"], case["maps"], case["orient_lines"], debug_break=None)
    pm, pang = S0.run(1)
    rows = orc.ang_prob_rows(S0, pm, pang)
    best = [rows[m][0]["orient"] for m in range(S0.nMaps)]
    second = [rows[m][1]["orient"] for m in range(S0.nMaps)]
    assert len(set(second)) == 1 and len(set(best)) == S0.nMaps and second[0] not in best
    M, H = second[0], best
    fill = [r for r in range(len(case["orient_lines"])) if r != M and r not in H]
    F = lambda n, k=0: [fill[(k + i) % len(fill)] for i in range(n)]           # noqa: E731
    blocks = [[M, fill[0], M] + F(11, 1), [M, M, M, M] + H + F(14 - 4 - len(H), 3), F(2, 5) + H + [M, M] + F(14 - 4 - len(H), 7)]
    order = [r for b in blocks for r in b]
    assert len(order) == 42 and all(len(b) == 14 for b in blocks)
    lines = []
    for i, r in enumerate(order):
        a = case["orient_lines"][r].split()
        lines.append("%12.8f%12.8f%12.8f%12.8f" % (float(a[0]), float(a[1]), float(a[2]), 0.05 + 0.02 * i))
    return dict(case, orient_lines=lines)


@pytest.fixture(scope="module")
def g11_rows():
    import oracle as orc
    case = g11_with_repeated_rows()
    S = orc.Setup(case["P"], case["model"], case["maps"], case["orient_lines"], debug_break=None)
    pm, pang = S.run(1)
    rows = orc.ang_prob_rows(S, pm, pang)
    K = int(S.pd.writeAngles)
    const = orc.logp_constant(S.pd)
    for m in range(S.nMaps):                                        # the case must be able to tell the rules apart
        keys = [float(np.log(pang[o, m]["forAngles"]) + pang[o, m]["ConstAngle"] + const) for o in range(S.nAngles)]
        ref = writer_heap(keys, K)
        assert [o for _, o in ref] == [r["orient"] for r in rows[m]]
        assert sum(1 for k in keys if k == ref[-1][0]) > 1, "no tie at the K-th key"
        narrow = merge_lists([shard_list(keys[a:b], a, K, K) for a, b in ((0, 14), (14, 28), (28, 42))], K)
        assert narrow != ref
    return case, S, rows


@pytest.mark.parametrize("shards", [1, 3])
def test_d_cli_on_a_list_with_repeated_rows(g11_rows, shards, tmp_path):
    import io_formats as iof
    from golden_util import write_case_inputs
    case, S, rows = g11_rows
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    cmd = [exe, "--Inputfile", os.path.join(case["dir"], "param.txt"), "--OutputFile", "out.txt"] + \
        write_case_inputs(case, tmp_path)
    env = dict(os.environ, BIOEM_ALGO="1", BIOEM_GPUS="1", BIOEM_SHARDS=str(shards))
    env.update(case["env"])
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    mine = iof.parse_ang_prob(str(tmp_path / "ANG_PROB"))
    pri = S.P["angprior"]
    for m in range(S.nMaps):
        assert len(mine[m]) == len(rows[m])
        for g, c in zip(rows[m], mine[m]):
            assert c["angles"] == [float("%.4f" % v) for v in S.angles[g["orient"]]][:len(c["angles"])], (m, g, c)
            assert c["sep"][-1] == float("%.4f" % pri[g["orient"]]), (m, g["orient"], c)      # WHICH copy: its prior
            assert abs(g["logp"] - c["logp"]) <= 5e-3
