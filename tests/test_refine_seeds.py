"""Seed selection for round-2 lists of different lengths (bioem_amd.refine.seed_lists) and the plan of the own-list pass
(bioem_hip_plan_own): no device needed."""
import ctypes as C
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# own instantiations that were left out of kernels_fast_own.hip (own_left_out): their shapes keep per-particle launches
LEFT_OUT = set()


def _cands(rows):
    from bioem_amd.engine import CANDIDATE_DTYPE
    out = np.zeros((len(rows), max(len(r) for r in rows)), dtype=CANDIDATE_DTYPE)
    out["orient"] = -1
    out["logp"] = -np.inf
    for p, r in enumerate(rows):
        for k, (o, l) in enumerate(r):
            out[p, k]["orient"] = o
            out[p, k]["logp"] = l
    return out


def test_seed_lists_on_hand_made_candidates():
    from bioem_amd import refine
    from bioem_amd.synthetic import random_quaternions
    angles = random_quaternions(12)
    grid = refine.local_grid(1, np.radians(4.0))
    G = len(grid)
    assert G == 27
    cands = _cands([
        [(3, -10.0), (7, -12.0), (1, -14.9), (5, -15.1)],   # window 5: three seeds; the fourth is outside
        [(2, -1.0), (4, -1.0), (6, -1.0), (8, -1.0)],       # all inside: max_seeds caps
        [(9, -3.0), (0, -30.0), (11, -3.5), (10, -40.0)],   # the window skips the second, takes the third
        [(-1, -5.0), (6, -50.0), (-1, -1.0), (2, -54.0)],   # orient = -1 is skipped; the first VALID one is the first seed
        [(5, -7.0), (-1, -np.inf), (-1, -np.inf), (-1, -np.inf)],
        [(-1, -np.inf)] * 4,                                # nothing owned: an empty list
    ])
    flat, off = refine.seed_lists(angles, cands, grid, max_seeds=3, log_window=5.0)
    seeds = [[3, 7, 1], [2, 4, 6], [9, 11], [6, 2], [5], []]
    assert flat.dtype == np.float32 and flat.shape == (sum(len(s) for s in seeds) * G, 4)
    assert off.dtype == np.int64 and list(off) == list(np.cumsum([0] + [len(s) * G for s in seeds]))
    for p, sd in enumerate(seeds):
        mine = flat[off[p]:off[p + 1]].reshape(len(sd), G, 4)
        for j, o in enumerate(sd):
            assert mine[j, 0].tobytes() == angles[o].astype(np.float32).tobytes()  # entry 0 of a block IS the seed
            assert np.array_equal(mine[j], refine.compose(angles[o:o + 1], grid)[0])
    # the first seed is always kept, whatever the window; max_seeds = 1 is refine_lists' single best
    flat0, off0 = refine.seed_lists(angles, cands, grid, max_seeds=4, log_window=0.0)
    assert list(np.diff(off0) // G) == [1, 4, 1, 1, 1, 0]
    flat1, off1 = refine.seed_lists(angles, cands[:5], grid, max_seeds=1)
    assert list(np.diff(off1)) == [G] * 5
    best = np.array([3, 2, 9, 6, 5])
    assert np.array_equal(flat1.reshape(5, G, 4), refine.compose(angles[best], grid))
    # no window: max_seeds alone decides
    _, offu = refine.seed_lists(angles, cands, grid, max_seeds=2)
    assert list(np.diff(offu) // G) == [2, 2, 2, 2, 1, 0]


def _plan(fn, N, d, g, algo):
    sig = C.create_string_buffer(256)
    assert fn(N, d, g, algo, sig, 256) == 0
    return sig.value.decode()


def test_plan_own():
    from bioem_amd.engine import load_library
    L = load_library()
    assert _plan(L.bioem_hip_plan, 224, 10, 1, 1) == "k_compare_fast<10, 16, false, 1>"
    assert _plan(L.bioem_hip_plan_own, 224, 10, 1, 1) == "k_compare_fast_own<10, 16, false, 1>"
    assert _plan(L.bioem_hip_plan_own, 128, 10, 1, 1).startswith("k_compare_fast_own<")  # the tutorial's size
    assert _plan(L.bioem_hip_plan_own, 224, 13, 1, 1) == "per particle: " + _plan(L.bioem_hip_plan, 224, 13, 1, 1)
    assert _plan(L.bioem_hip_plan_own, 75, 10, 1, 1) == "per particle: " + _plan(L.bioem_hip_plan, 75, 10, 1, 1)
    sig = C.create_string_buffer(256)
    assert L.bioem_hip_plan_own(224, 200, 1, 1, sig, 256) == 2
    n_fast = 0
    with gzip.open(os.path.join(ROOT, "tests", "golden", "selection_snapshot.txt.gz"), "rt") as f:
        for ln in f:
            N, d, g, algo, want = ln.rstrip("\n").split(" ", 4)
            own = _plan(L.bioem_hip_plan_own, int(N), int(d), int(g), int(algo))
            if want.startswith("k_compare_fast<") and " x " not in want and want not in LEFT_OUT:
                assert own == want.replace("k_compare_fast<", "k_compare_fast_own<"), ln
                n_fast += 1
            else:
                assert own == "per particle: " + want, ln
    assert n_fast > 0
