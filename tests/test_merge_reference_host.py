"""The merge of shards on the host, entry by entry against tests/merge_reference.py (no GPU): bioem_hip_merge_host on map
entries and on full angle tables, merge_ctf_tables, bioem_hip_merge_topk_host_wide, and merge_prob_maps over gloo with
three ranks.  tests/test_merge_exact_gpu.py runs the same cases through the device's half (k_merge_shards, k_topk_angles).

Map entries: Constoadd and the six record fields are the winning shard's bit for bit (the LOWEST shard holding the
largest Constoadd), |log(Total) + Constoadd - log P| <= B (merge_reference.bound, derived from the operations), Total is
exactly 0 where nothing was folded into any shard.  Cases (merge_cases.map_cases) for S = 1, 2, 3, 8, 64 shards.

Candidate lists: the merge of the shards' lists of width 2K - 1 (merge_reference.shard_list) must be writer_heap of the
whole table -- all 3^8 key patterns over {-inf, 0, 1}, K = 1 ... 4, every cut into two and three shards; 200 random
tables of 40 orientations over five key values cut into 1 ... 7 shards -- with every field of every candidate its table
entry's, and unused slots (0, MIN_PROB, -inf, -1).  With K-wide lists the exhaustive test fails (test_k_wide_lists_are_
not_enough counts the 2 063 (pattern, K) pairs the brute force found): that is what the K-wide merge computed before
the wide lists existed.

Largest |d log P| / B (every test prints its own): 0.000 with one shard (the one product is exact), 0.103 with 2, 0.226
with 3, 0.128 with 8, 0.066 with 64; the same for map entries, angle tables, CTF tables and the three gloo ranks.

The reference's own slips (ties to the highest shard, `<=` in the heap, K-wide lists) fail these tests:
test_slips_of_the_reference_fail."""
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import merge_cases as mc
from merge_reference import MIN_PROB, merge_lists, shard_list, writer_heap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS = [1, 2, 3, 8, 64]


def _eng():
    import bioem_amd.engine as eng
    return eng


# ------------------------------------------------------------------------------------------------------
# the reference against itself
# ------------------------------------------------------------------------------------------------------
def test_closed_rule_is_the_writers_heap():
    """shard_list restates the rule in closed form: its first K slots are writer_heap of the block, for every pattern"""
    for K in (1, 2, 3, 4):
        for pat in mc.exhaustive_patterns():
            want = writer_heap(pat, K)
            for W in (K, 2 * K - 1):
                got = shard_list(pat, 0, K, W)
                assert got[:K] == want + [None] * (K - len(want)), (pat, K)
                extra = [x for x in got[K:] if x is not None]
                assert extra == sorted(extra, key=lambda x: x[1]) and got[K:] == extra + [None] * (W - K - len(extra))


def test_reference_example_of_the_issue():
    """K = 2, keys 5 5 5 7: the serial walk ends with {7(3), 5(1)}; the K-wide merge after a cut at 1 gives 5(2)"""
    keys = (5.0, 5.0, 5.0, 7.0)
    assert writer_heap(keys, 2) == [(7.0, 3), (5.0, 1)]
    narrow = [shard_list(keys[:1], 0, 2, 2), shard_list(keys[1:], 1, 2, 2)]
    assert merge_lists(narrow, 2) == [(7.0, 3), (5.0, 2)]
    wide = [shard_list(keys[:1], 0, 2, 3), shard_list(keys[1:], 1, 2, 3)]
    assert wide[1] == [(7.0, 3), (5.0, 2), (5.0, 1)]
    assert merge_lists(wide, 2) == [(7.0, 3), (5.0, 1)]


# ------------------------------------------------------------------------------------------------------
# map entries
# ------------------------------------------------------------------------------------------------------
def _merge_maps(blocks):
    eng = _eng()
    S, n = blocks.shape
    raw = [np.ascontiguousarray(blocks[s]).view(np.uint8).reshape(-1) for s in range(S)]
    return eng.merge_host(raw, n, 0, 0).view(eng.PROB_MAP_DTYPE)


@pytest.mark.parametrize("S", SHARDS)
def test_merge_host_map_entries(S):
    cases = mc.map_cases(S)
    blocks = mc.pack_maps(cases, S)
    worst = mc.check_maps(_merge_maps(blocks), blocks, cases)
    print("merge_host, %d shards, %d entries: largest |d log P| / B = %.3f" % (S, len(cases), worst))


@pytest.mark.parametrize("S", SHARDS)
def test_merge_host_full_angle_tables(S):
    """writeAngles: the CTF-split use, every shard holds every orientation's entry.  nAngles = 3 rows of the cases, each row
    rotated, behind map entries of their own"""
    eng = _eng()
    cases = mc.map_cases(S)
    n, nA = len(cases), 3
    maps = mc.pack_maps(cases, S)
    rows = [mc.pack_angles(cases, S, first=5 * a + 1) for a in range(nA)]
    raw = []
    for s in range(S):
        ang = np.stack([rows[a][s] for a in range(nA)])                       # [nA][n], orientation-major
        raw.append(np.concatenate([maps[s].view(np.uint8).reshape(-1), ang.view(np.uint8).reshape(-1)]))
    out = eng.merge_host(raw, n, nA, 1)
    worst = mc.check_maps(out[:n * 40].view(eng.PROB_MAP_DTYPE), maps, cases)
    pang = out[n * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(nA, n)
    for a in range(nA):
        worst = max(worst, mc.check_maps(pang[a], rows[a], cases, first=5 * a + 1, records=False))
    print("merge_host with angle tables, %d shards: largest |d log P| / B = %.3f" % (S, worst))


@pytest.mark.parametrize("S", SHARDS)
def test_merge_ctf_tables(S):
    eng = _eng()
    cases = mc.map_cases(S)
    nCTF, nMaps = 3, (len(cases) + 2) // 3
    blocks = mc.pack_maps(cases, S, n=nCTF * nMaps)
    merged = eng.merge_ctf_tables([blocks[s].reshape(nCTF, nMaps) for s in range(S)])
    assert merged.shape == (nCTF, nMaps)
    worst = mc.check_maps(merged.reshape(-1), blocks, cases)
    print("merge_ctf_tables, %d shards: largest |d log P| / B = %.3f" % (S, worst))


# ------------------------------------------------------------------------------------------------------
# candidate lists
# ------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _exhaustive(wide, slip=None, Ks=(1, 2, 3, 4)):
    """number of (pattern, K) pairs for which some cut into two or three shards merges to something else than
    writer_heap of the whole pattern"""
    eng = _eng()
    pats = mc.exhaustive_patterns()
    T = len(pats[0])
    wrong = 0
    for K in Ks:
        W = 2 * K - 1 if wide else K
        seg = mc.SegmentLists(pats, K, W)
        want = mc.expected_topk(pats, K, slip)
        bad = np.zeros(len(pats), dtype=bool)
        for nShards in (2, 3):
            for cut in mc.cuts(T, nShards):
                lists = [seg.block(a, b) for a, b in zip(cut, cut[1:])]
                got = eng.merge_topk_host(lists, K)
                if not _same(got, want):
                    bad |= np.array([not _same(g, w) for g, w in zip(got, want)])
        wrong += int(bad.sum())
    return wrong


def test_wide_lists_merge_to_the_writers_walk_exhaustive():
    assert _exhaustive(wide=True) == 0


def test_k_wide_lists_are_not_enough():
    """the same test on K-wide lists: the library's K-wide merge (what every merge was before the wide lists) is wrong
    for exactly the (pattern, K) pairs of the brute force, none of them at K = 1"""
    assert _exhaustive(wide=False, Ks=(1,)) == 0
    assert _exhaustive(wide=False) == 2063


def test_wide_lists_random_tables():
    eng = _eng()
    tables = mc.random_tables()
    nO = len(tables[0])
    rng = random.Random(20261022)
    small = empty = 0
    for nShards in range(1, 8):
        for K in (1, 2, 5, 10):
            W = 2 * K - 1
            cutsets = []
            for p in range(len(tables)):
                cut = list(mc.random_cut(rng, nO, nShards))
                if nShards > 2 and p % 3 == 0:
                    cut[2] = cut[1]                                       # an empty shard
                if nShards > 1 and p % 3 == 1:
                    cut[1] = min(cut[2], cut[0] + rng.randint(1, 3))      # a shard of one to three orientations
                cutsets.append(cut)
                lens = [b - a for a, b in zip(cut, cut[1:])]
                empty += 0 in lens
                small += any(0 < n < K for n in lens)
            lists = [np.stack([mc.pack_list(shard_list(t[c[s]:c[s + 1]], c[s], K, W), W) for t, c in zip(tables, cutsets)])
                     for s in range(nShards)]
            got = eng.merge_topk_host(lists, K)
            want = mc.expected_topk(tables, K)
            for p in range(len(tables)):
                assert [int(o) for o in got[p]["orient"]] == [int(o) for o in want[p]["orient"]], (nShards, K, p)
            assert _same(got, want)
            if nShards == 1:                                              # K-wide lists of ONE shard are the writer's too
                assert _same(eng.merge_topk_host([np.ascontiguousarray(lists[0][:, :K])]), want)
    assert small > 100 and empty > 100


def test_unused_slots_and_refusals():
    eng = _eng()
    K, W = 4, 7
    tables = [(1.0, mc.NINF), ()]                                         # two orientations, and none at all
    lists = [np.stack([mc.pack_list(shard_list(t, 0, K, W), W) for t in tables])]
    got = eng.merge_topk_host(lists, K)
    assert [int(o) for o in got[0]["orient"]] == [0, 1, -1, -1]
    assert got[0]["logp"][1] == mc.NINF and got[0]["ConstAngle"][1] == MIN_PROB      # a fresh entry is a candidate too
    for c in list(got[0][2:]) + list(got[1]):
        assert (c["forAngles"], c["ConstAngle"], c["logp"], c["orient"], c["pad"]) == (0.0, MIN_PROB, mc.NINF, -1, 0)
    L = eng.load_library()
    import ctypes as C
    arr = (C.c_void_p * 1)(lists[0].ctypes.data)
    out = np.zeros((2, K), dtype=eng.CANDIDATE_DTYPE)
    po = out.ctypes.data_as(C.c_void_p)
    assert L.bioem_hip_merge_topk_host_wide(0, 2, K, W, arr, po) == 2
    assert L.bioem_hip_merge_topk_host_wide(1, 2, 0, W, arr, po) == 2
    assert L.bioem_hip_merge_topk_host_wide(1, 2, K, K - 1, arr, po) == 2
    assert L.bioem_hip_merge_topk_host_wide(1, 2, K, W, None, po) == 2
    assert L.bioem_hip_merge_topk_host_wide(1, 2, K, W, arr, None) == 2
    assert L.bioem_hip_merge_topk_host_wide(1, 2, K, W, arr, po) == 0 and _same(out, got)


# ------------------------------------------------------------------------------------------------------
# the slips of the reference
# ------------------------------------------------------------------------------------------------------
def test_slips_of_the_reference_fail():
    for S in (2, 3, 8):
        cases = mc.map_cases(S)
        blocks = mc.pack_maps(cases, S)
        merged = _merge_maps(blocks)
        with pytest.raises(AssertionError):
            mc.check_maps(merged, blocks, cases, slip="highest")
    assert _exhaustive(wide=True, slip="le", Ks=(2,)) > 0
    assert _exhaustive(wide=False, Ks=(2,)) > 0                           # the K-wide slip, see test_k_wide_lists_are_not_enough


# ------------------------------------------------------------------------------------------------------
# merge_prob_maps over gloo, three ranks
# ------------------------------------------------------------------------------------------------------
GLOO_K = 3


def _gloo_inputs():
    cases = mc.map_cases(3)
    blocks = mc.pack_maps(cases, 3)
    n = len(cases)
    tables = mc.random_tables(count=n, nO=12, seed=20261023, values=(mc.NINF, 0.0, 1.0))
    rng = random.Random(20261024)
    cutsets = [mc.random_cut(rng, 12, 3) for _ in range(n)]
    W = 2 * GLOO_K - 1
    lists = [np.stack([mc.pack_list(shard_list(t[c[s]:c[s + 1]], c[s], GLOO_K, W), W) for t, c in zip(tables, cutsets)])
             for s in range(3)]
    return cases, blocks, tables, lists


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, outdir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist
    from bioem_amd.dist_merge import merge_prob_maps
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, blocks, _, lists = _gloo_inputs()
    merged, cands = merge_prob_maps(blocks[rank], torch.device("cpu"), cands=lists[rank], K=GLOO_K)
    alone = merge_prob_maps(blocks[rank], torch.device("cpu"))
    assert alone.tobytes() == merged.tobytes()
    np.save(os.path.join(outdir, "merged_%d.npy" % rank), merged)
    np.save(os.path.join(outdir, "cands_%d.npy" % rank), cands)
    dist.barrier()
    dist.destroy_process_group()


def test_merge_prob_maps_three_ranks_over_gloo(tmp_path):
    mp.spawn(_gloo_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    cases, blocks, tables, _ = _gloo_inputs()
    merged = [np.load(tmp_path / ("merged_%d.npy" % r)) for r in range(3)]
    cands = [np.load(tmp_path / ("cands_%d.npy" % r)) for r in range(3)]
    for r in (1, 2):
        assert _same(merged[r], merged[0]) and _same(cands[r], cands[0])
    worst = mc.check_maps(merged[0], blocks, cases)
    assert cands[0].shape == (len(cases), GLOO_K)
    assert _same(cands[0], mc.expected_topk(tables, GLOO_K))
    print("merge_prob_maps, 3 ranks: largest |d log P| / B = %.3f" % worst)
