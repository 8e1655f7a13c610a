#!/usr/bin/env python3
"""Time of bioem_hip_orientation_sums against bioem_hip_topk_angles (K = 10), the only other consumer of the angle table,
over the same table: 36 864 orientations (BASELINE config 5) x 1 000 particles, 590 MB.  The handle is a small one (32
pixels): neither call looks at an image; the table is drawn here and goes in through start_run, the quaternions are
random.  One process, one device, the two calls alternating after one warm-up call each (buffers, code load); medians
over the repeats.  Both calls end in a stream synchronisation and a small copy (136 KB, 320 KB), so the wall time of
the call is the device time plus that; for the orientation sums the engine's own phase record (HIP events around its
five launches) is printed beside it, and the table's bytes, read twice, against the 8 TB/s the HBM is specified with and
the 6.3 TB/s a copy kernel reaches.  -> profiles/orient_stats_measure.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--orientations", type=int, default=36864)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--euler", action="store_true", help="Euler-angle list: no moments")
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import make_param_device
    nO, nP = a.orientations, a.particles
    pd = make_param_device(32, 3, 1, nO, (1.0, 1.0, 1.0), 1, 2.0)
    pd.writeAngles = 10
    E = eng.Engine(pd, nP, nO, 1, algo=1, device=0)
    rng = np.random.default_rng(1)
    E.upload_orientations(rng.standard_normal((nO, 4)).astype(np.float32), not a.euler)
    raw, _, pang = eng.new_prob_block(nP, nO, 10)
    # a posterior that is neither pinned nor flat: a few hundred orientations within some log units of the best
    pang["forAngles"] = rng.uniform(0.5, 2.0, (nO, nP))
    pang["ConstAngle"] = rng.uniform(-300.0, 400.0, nP)[None, :] - rng.exponential(40.0, (nO, nP))
    E.start_run(raw)
    E.finish_run(raw)
    table = nO * nP * 16
    print("%d orientations x %d particles, %.0f MB of table, %s" % (nO, nP, 1e-6 * table,
                                                                   "Euler angles" if a.euler else "quaternions"))
    first = E.orientation_sums()
    E.topk_angles(10, 0.0)
    t = {"sums": [], "sums_dev": [], "topk": []}
    for r in range(a.repeats):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        out = E.orientation_sums()
        t["sums"].append(1e3 * (time.perf_counter() - t0))
        t["sums_dev"].append(1e3 * E.phase_records()["seconds"].sum())
        E.set_phase_timing(False)
        assert out.tobytes() == first.tobytes()
        t0 = time.perf_counter()
        E.topk_angles(10, 0.0)
        t["topk"].append(1e3 * (time.perf_counter() - t0))
        print("run %d: orientation_sums %.3f ms wall, %.3f ms on the device; topk_angles (K = 10) %.3f ms wall"
              % (r, t["sums"][-1], t["sums_dev"][-1], t["topk"][-1]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in ("sums", "sums_dev", "topk"):
        print("%-8s: median %.3f ms, min %.3f, max %.3f over %d runs" % (k, med[k], min(t[k]), max(t[k]), len(t[k])))
    print("WALL time of the call, orientation_sums / topk_angles (medians; topk_angles has no phase record, so no ratio of "
          "device times is formed): %.3f" % (med["sums"] / med["topk"]))
    for name, bw in (("8.0 TB/s (specified)", 8.0e12), ("6.3 TB/s (copy kernel)", 6.3e12)):
        floor = 1e3 * 2 * table / bw
        print("2 x table bytes at %s: %.3f ms; device time / that: %.2f" % (name, floor, med["sums_dev"] / floor))
    from bioem_amd import orient_stats
    st = orient_stats.derive(first)
    print("the posteriors drawn: nEff median %.1f, entropy median %.2f nats" % (np.median(st["nEff"]), np.median(st["entropy"])))
    E.close()


if __name__ == "__main__":
    main()
