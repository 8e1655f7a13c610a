"""Inputs of the merge tests (tests/test_merge_reference_host.py, tests/test_merge_exact_gpu.py): the cases as plain
Python numbers, and their packing into the byte layouts the merges read.  numpy only packs and compares here; the
expected values come from tests/merge_reference.py."""
import itertools
import math
import random

import numpy as np

from bioem_amd.engine import CANDIDATE_DTYPE, PROB_ANGLE_DTYPE, PROB_MAP_DTYPE
from merge_reference import MIN_PROB, bound, merge_entry, share, shard_list, writer_heap

NINF = float("-inf")
RECORD = ("cent_x", "cent_y", "orient", "conv", "norm", "mu")
SPREADS = (0.0, "spacing", 30.0, 700.0, 740.0, 750.0)
FRESH = (0.0, MIN_PROB)


# ------------------------------------------------------------------------------------------------------
# map entries
# ------------------------------------------------------------------------------------------------------
def _full_mantissa(rng, lo, hi):
    return rng.uniform(lo, hi)             # 53 random bits scaled into [lo, hi): no trailing zeros to speak of


def map_cases(S, seed=20261020):
    """[(name, Total[S], Constoadd[S])]: Constoadd in [-3000, -1000], Total in [1, 1e4]; ties of Constoadd between the
    shards {0, 1}, {1, 2}, {0, S-1} and all; a fresh shard (0, MIN_PROB) at every position and everywhere; one shard at C
    and the others `spread` below it, for the SPREADS and for the 10^6 of fresh shards"""
    rng = random.Random(seed + S)

    def draw():
        return ([_full_mantissa(rng, 1.0, 1e4) for _ in range(S)], [_full_mantissa(rng, -3000.0, -1000.0) for _ in range(S)])

    cases = [("random",) + draw()]
    for tie in ({0, 1}, {1, 2}, {0, S - 1}, set(range(S))):
        if max(tie) >= S or (len(tie) < 2 and S > 1):
            continue
        T, C = draw()
        top = max(C) + 1.0 + rng.random()                   # the tied shards hold the maximum
        for s in tie:
            C[s] = top
        cases.append(("tie %s" % sorted(tie), T, C))
        if len(tie) < S:                                    # and a tie below the maximum moves nothing
            T, C = draw()
            low = min(C) - 1.0 - rng.random()
            for s in tie:
                C[s] = low
            cases.append(("low tie %s" % sorted(tie), T, C))
    for s in range(S):
        T, C = draw()
        T[s], C[s] = FRESH
        cases.append(("fresh %d" % s, T, C))
    cases.append(("all fresh", [0.0] * S, [MIN_PROB] * S))
    for spread in SPREADS:
        for who in sorted({0, S - 1, S // 2}):
            T, C = draw()
            top = C[who]
            below = top - spread if spread != "spacing" else math.nextafter(top, NINF)
            C = [top if s == who else below for s in range(S)]
            cases.append(("spread %s, top %d" % (spread, who), T, C))
    for who in sorted({0, S - 1}):
        T, C = draw()
        cases.append(("the rest fresh, top %d" % who, [T[s] if s == who else 0.0 for s in range(S)],
                      [C[s] if s == who else MIN_PROB for s in range(S)]))
    return cases


def pack_maps(cases, S, n=None, first=0):
    """blocks[S][n] of PROB_MAP_DTYPE: entry i is case (first + i) mod len(cases); the record of shard s at entry i is its
    own (a fresh shard's is zero, as start_run leaves it)"""
    n = len(cases) if n is None else n
    blocks = np.zeros((S, n), dtype=PROB_MAP_DTYPE)
    for i in range(n):
        _, T, C = cases[(first + i) % len(cases)]
        for s in range(S):
            e = blocks[s, i]
            e["Total"], e["Constoadd"] = T[s], C[s]
            if (T[s], C[s]) != FRESH:
                e["cent_x"], e["cent_y"], e["orient"], e["conv"] = 3 * s + 1, -(s + 2), 1000 * s + i, s + 7
                e["norm"], e["mu"] = 1.5 + s, -0.25 * s - i
    return blocks


def pack_angles(cases, S, n=None, first=0):
    """the same cases as angle-table entries: [S][n] of PROB_ANGLE_DTYPE"""
    n = len(cases) if n is None else n
    out = np.zeros((S, n), dtype=PROB_ANGLE_DTYPE)
    for i in range(n):
        _, T, C = cases[(first + i) % len(cases)]
        out["forAngles"][:, i] = T
        out["ConstAngle"][:, i] = C
    return out


def check_maps(merged, blocks, cases, first=0, records=True, slip=None):
    """the assertions on merged map entries (or angle entries: records = False); returns the largest |d log P| / B"""
    S, n = blocks.shape
    tot_f, con_f = ("Total", "Constoadd") if records else ("forAngles", "ConstAngle")
    worst = 0.0
    for i in range(n):
        name, T, C = cases[(first + i) % len(cases)]
        ref = merge_entry(T, C, slip)
        got = merged[i]
        assert np.float64(got[con_f]).tobytes() == np.float64(ref.Constoadd).tobytes(), (name, i)
        if records:
            for f in RECORD:
                assert got[f].tobytes() == blocks[ref.winner, i][f].tobytes(), (name, i, f, ref.winner)
        if all(t == 0.0 for t in T):
            assert got[tot_f] == 0.0 and not np.signbit(got[tot_f]), (name, i)
            continue
        assert got[tot_f] > 0.0, (name, i)
        r = share(got[tot_f], got[con_f], T, C)
        assert r <= 1.0, (name, i, r, float(bound(T, C)))
        worst = max(worst, r)
    return worst


# ------------------------------------------------------------------------------------------------------
# candidate lists
# ------------------------------------------------------------------------------------------------------
NUMCONST = -100.0                          # an integer: with forAngles = 1 and an integer ConstAngle the key is exact


def entry_of(key):
    """(forAngles, ConstAngle) of the table entry whose key under NUMCONST is `key`: the fresh entry for -inf"""
    return (0.0, MIN_PROB) if key == NINF else (1.0, key - NUMCONST)


def exhaustive_patterns(T=8, values=(NINF, 0.0, 1.0)):
    return list(itertools.product(values, repeat=T))


def cuts(T, nShards):
    """every way to cut T orientations into nShards consecutive blocks (empty ones included): the block borders"""
    return [(0,) + c + (T,) for c in itertools.combinations_with_replacement(range(T + 1), nShards - 1)]


def pack_table(patterns):
    """[nO][nMaps] PROB_ANGLE_DTYPE: particle p's keys are patterns[p]"""
    nO = len(patterns[0])
    tab = np.zeros((nO, len(patterns)), dtype=PROB_ANGLE_DTYPE)
    for p, pat in enumerate(patterns):
        for o, k in enumerate(pat):
            tab[o, p] = entry_of(k)
    return tab


def pack_list(lst, W):
    """one shard_list as [W] CANDIDATE_DTYPE"""
    out = np.zeros(W, dtype=CANDIDATE_DTYPE)
    for j, x in enumerate(lst):
        if x is None:
            out[j] = (0.0, MIN_PROB, NINF, -1, 0)
        else:
            out[j] = entry_of(x[0]) + (x[0], x[1], 0)
    return out


class SegmentLists:
    """shard_list of every block [a, b) of every pattern, packed: one row per DISTINCT run of keys, looked up per pattern
    (6 561 patterns share 3^(b-a) runs)"""

    def __init__(self, patterns, K, W):
        self.patterns, self.K, self.W = patterns, K, W
        self._rows = {}

    def block(self, a, b):
        """[nMaps][W] CANDIDATE_DTYPE of the shard that owns orientations a ... b-1"""
        if (a, b) not in self._rows:
            runs, index = {}, np.zeros(len(self.patterns), dtype=np.int64)
            for p, pat in enumerate(self.patterns):
                index[p] = runs.setdefault(pat[a:b], len(runs))
            rows = np.zeros((len(runs), self.W), dtype=CANDIDATE_DTYPE)
            for run, r in runs.items():
                rows[r] = pack_list(shard_list(run, a, self.K, self.W), self.W)
            self._rows[(a, b)] = (rows, index)
        rows, index = self._rows[(a, b)]
        return np.ascontiguousarray(rows[index])


def expected_topk(patterns, K, slip=None):
    """[nMaps][K] CANDIDATE_DTYPE: writer_heap of every whole pattern"""
    out = np.zeros((len(patterns), K), dtype=CANDIDATE_DTYPE)
    cache = {}
    for p, pat in enumerate(patterns):
        if pat not in cache:
            got = writer_heap(pat, K, slip)
            cache[pat] = pack_list(got + [None] * (K - len(got)), K)
        out[p] = cache[pat]
    return out


def random_tables(count=200, nO=40, seed=20261021, values=(NINF, -2.0, 0.0, 1.0, 3.0)):
    rng = random.Random(seed)
    return [tuple(rng.choice(values) for _ in range(nO)) for _ in range(count)]


def random_cut(rng, T, nShards):
    return (0,) + tuple(sorted(rng.randint(0, T) for _ in range(nShards - 1))) + (T,)
