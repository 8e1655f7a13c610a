#!/usr/bin/env python3
"""Device time of bioem_hip_orientation_occupancy (B) against bioem_hip_orientation_sums (A), the other full pass over the
angle table, on the same table: 36 864 orientations (BASELINE config 5) x 1 000 particles, 590 MB, quaternions.  The handle
is a small one (32 pixels): neither call looks at an image; the table is drawn here and goes in through start_run.  One
process, one device, the two calls alternating after one warm-up call each (buffers, code load); medians over the repeats,
from the engine's own phase records (HIP events around each call's launches), the wall time of the calls beside them.
A reads the table twice (maximum, then sums), B once: the table's bytes against the 8 TB/s the HBM is specified with and
the 6.3 TB/s a copy kernel reaches are printed for both.  -> profiles/orient_occupancy_measure.txt"""
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
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd import orient_occupancy
    from bioem_amd.synthetic import make_param_device
    nO, nP = a.orientations, a.particles
    pd = make_param_device(32, 3, 1, nO, (1.0, 1.0, 1.0), 1, 2.0)
    pd.writeAngles = 10
    E = eng.Engine(pd, nP, nO, 1, algo=1, device=0)
    rng = np.random.default_rng(1)
    E.upload_orientations(rng.standard_normal((nO, 4)).astype(np.float32), True)
    raw, _, pang = eng.new_prob_block(nP, nO, 10)
    # a posterior that is neither pinned nor flat: a few hundred orientations within some log units of the best
    pang["forAngles"] = rng.uniform(0.5, 2.0, (nO, nP))
    pang["ConstAngle"] = rng.uniform(-300.0, 400.0, nP)[None, :] - rng.exponential(40.0, (nO, nP))
    E.start_run(raw)
    E.finish_run(raw)
    table = nO * nP * 16
    print("%d orientations x %d particles, %.0f MB of table, quaternions" % (nO, nP, 1e-6 * table))
    sums = E.orientation_sums()
    first = E.orientation_occupancy(sums)
    E.set_phase_timing(True)        # warm-up of the timed path too: the first call with phase records creates its events
    E.orientation_sums()
    E.orientation_occupancy(sums)
    E.phase_records()
    E.set_phase_timing(False)
    t = {"A_dev": [], "A_wall": [], "B_dev": [], "B_wall": []}
    for r in range(a.repeats):
        for key, call in (("A", lambda: E.orientation_sums()), ("B", lambda: E.orientation_occupancy(sums))):
            E.set_phase_timing(True)
            t0 = time.perf_counter()
            out = call()
            t[key + "_wall"].append(1e3 * (time.perf_counter() - t0))
            t[key + "_dev"].append(1e3 * E.phase_records()["seconds"].sum())
            E.set_phase_timing(False)
            assert out.tobytes() == (sums if key == "A" else first).tobytes()
        print("run %d: A orientation_sums %.3f ms on the device (%.3f wall); B orientation_occupancy %.3f ms on the device "
              "(%.3f wall)" % (r, t["A_dev"][-1], t["A_wall"][-1], t["B_dev"][-1], t["B_wall"][-1]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in ("A_dev", "A_wall", "B_dev", "B_wall"):
        print("%-6s: median %.3f ms, min %.3f, max %.3f over %d runs" % (k, med[k], min(t[k]), max(t[k]), len(t[k])))
    print("device time B / A (medians): %.3f" % (med["B_dev"] / med["A_dev"]))
    for name, bw in (("8.0 TB/s (specified)", 8.0e12), ("6.3 TB/s (copy kernel)", 6.3e12)):
        floor = 1e3 * table / bw
        print("table bytes at %s: %.3f ms; B / that: %.2f; A / twice that: %.2f"
              % (name, floor, med["B_dev"] / floor, med["A_dev"] / (2 * floor)))
    per, ds = orient_occupancy.derive(first, int(orient_occupancy.counted(sums).sum()))
    print("the data set drawn: %d particles counted, %.1f effective views of %d, largest fraction %.3g"
          % (ds["nCounted"], ds["nEffViews"], nO, ds["maxFraction"]))
    E.close()


if __name__ == "__main__":
    main()
