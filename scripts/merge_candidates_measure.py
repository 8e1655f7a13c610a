#!/usr/bin/env python3
"""Time of Engine.merge_candidates (lists of 2K - 1: the K best and the tie candidates, two walks over the angle table)
against Engine.topk_angles (K-wide, one walk) at K = 10 over the same table: 4 608 orientations x 1 000 particles, 74 MB,
by the method of scripts/orient_stats_measure.py.  The handle is a small one (32 pixels): neither call looks at an image;
the table is drawn here and goes in through start_run.  One process, one device, the two calls alternating after one
warm-up call each; medians over the repeats.  Both calls end in a stream synchronisation and a copy to the host (320 KB,
608 KB), so the wall time is the device time plus that.  --tree names another checkout (built) whose package is loaded
instead: a tree without merge_candidates (the parent commit) times topk_angles alone.  --ties draws every row three
times, so that the K-th key is a tie for every particle (K = 10: three best rows and one of the fourth's three copies)
and the second walk has candidates to write.
-> profiles/merge_candidates_measure.txt"""
import argparse
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--orientations", type=int, default=4608)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--ties", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import make_param_device
    nO, nP, K = a.orientations, a.particles, a.K
    pd = make_param_device(32, 3, 1, nO, (1.0, 1.0, 1.0), 1, 2.0)
    pd.writeAngles = K
    E = eng.Engine(pd, nP, nO, 1, algo=1, device=0)
    rng = np.random.default_rng(1)
    raw, _, pang = eng.new_prob_block(nP, nO, K)
    rows = nO // 3 if a.ties else nO
    F = rng.uniform(0.5, 2.0, (rows, nP))
    C = rng.uniform(-300.0, 400.0, nP)[None, :] - rng.exponential(40.0, (rows, nP))
    if a.ties:
        F, C = np.repeat(F, 3, axis=0), np.repeat(C, 3, axis=0)
        assert len(F) == nO, "--ties wants a multiple of three orientations"
    pang["forAngles"], pang["ConstAngle"] = F, C
    E.start_run(raw)
    E.finish_run(raw)
    wide = hasattr(E, "merge_candidates")
    print("tree %s: %d orientations x %d particles, %.0f MB of table, K = %d%s" %
          (a.tree, nO, nP, 1e-6 * nO * nP * 16, K, ", every row three times" if a.ties else ""))
    first = E.topk_angles(K, 0.0)
    t = {"topk_angles": []}
    if wide:
        cand = E.merge_candidates(K, 0.0)
        assert cand[:, :K].tobytes() == first.tobytes()
        print("tie candidates written: %d of %d slots" % (int((cand[:, K:]["orient"] >= 0).sum()), cand[:, K:].size))
        t["merge_candidates"] = []
    for r in range(a.repeats):
        t0 = time.perf_counter()
        out = E.topk_angles(K, 0.0)
        t["topk_angles"].append(1e3 * (time.perf_counter() - t0))
        assert out.tobytes() == first.tobytes()
        if wide:
            t0 = time.perf_counter()
            out = E.merge_candidates(K, 0.0)
            t["merge_candidates"].append(1e3 * (time.perf_counter() - t0))
            assert out.tobytes() == cand.tobytes()
    for k, v in t.items():
        print("%-16s: median %.3f ms, min %.3f, max %.3f over %d runs (wall time of the call)" %
              (k, float(np.median(v)), min(v), max(v), len(v)))
    if wide:
        print("merge_candidates / topk_angles (medians): %.2f" %
              (float(np.median(t["merge_candidates"])) / float(np.median(t["topk_angles"]))))
    E.close()


if __name__ == "__main__":
    main()
