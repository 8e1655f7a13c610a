#!/usr/bin/env python3
"""Device time of bioem_hip_view_sums against bioem_hip_best_match_rings over the same records on the config-2 workload
(224^2, 1 000 particles, 5 CTFs): the engine's own phase records (HIP events on the stream).  A = best_match_rings (phase 0
projection, phase 2 the particle spectra's way back to reference layout and the ring pass: it reads the same spectra);
B = view_sums (phase 2: the same way back and the accumulation), once with the records grouped by orientation (--views
distinct orientations, so a view holds about particles / views members spread over all particle batches) and once with all
records in one group, which exposes the latency of one lane's serial walk over its members.  One process, one device,
the three calls alternating; the first call of each (staging buffers, code load) is not counted; medians over --repeats
runs.  The bytes B must read are the particle spectra, once; the floor is that over the 6.3 TB/s a copy kernel reaches
on this device.  The particles are noise images (the pass does not depend on what they hold), the records drawn here.
-> profiles/view_averages_measure.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.3e12  # bytes per second of a copy kernel on one MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=224)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--orientations", type=int, default=4608)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd import view_average as va
    from bioem_amd.synthetic import Workload
    W = Workload(N=a.pixels, nP=a.particles, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    rng = np.random.default_rng(1)
    E.upload_particle_maps(rng.standard_normal((a.particles, a.pixels, a.pixels)).astype(np.float32))
    rec = np.zeros(a.particles, dtype=eng.PROB_MAP_DTYPE)
    rec["Total"] = 1.0
    rec["orient"] = rng.choice(a.orientations, a.views, replace=False)[rng.integers(0, a.views, a.particles)]
    rec["conv"] = rng.integers(0, W.nCTF, a.particles)
    rec["cent_x"] = rng.integers(-10, 11, a.particles)
    rec["cent_y"] = rng.integers(-10, 11, a.particles)
    rec["norm"], rec["mu"] = 0.01, -0.02
    grouped, orient = va.groups_by_orientation(rec, 1)
    one = np.zeros(a.particles, dtype=np.int32)
    M = a.pixels * (a.pixels // 2 + 1)
    must = 8.0 * M * a.particles
    print("%d records at %d^2, %d CTFs on the handle, particle batches of %d; %d views of %d..%d particles; the spectra are "
          "%.1f MB: %.3f ms at 6.3 TB/s" % (a.particles, a.pixels, W.nCTF, E.max_batch()[0], len(orient),
                                            np.bincount(grouped).min(), np.bincount(grouped).max(), 1e-6 * must,
                                            1e3 * must / COPY_RATE))
    calls = (("A rings", lambda: E.best_match_rings(rec)), ("B grouped", lambda: E.view_sums(rec, grouped)),
             ("B one group", lambda: E.view_sums(rec, one)))
    first = [c() for _, c in calls]  # first calls: staging buffers, code load
    tot = {k: [] for k, _ in calls}
    ring = []
    for r in range(a.repeats):
        for i, (what, call) in enumerate(calls):
            E.set_phase_timing(True)
            t0 = time.perf_counter()
            out = call()
            wall = time.perf_counter() - t0
            ph = E.phase_records()
            E.set_phase_timing(False)
            s = [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(3)]
            tot[what].append(sum(s))
            if i == 0:
                ring.append(s[2])
                assert out.tobytes() == first[0].tobytes()
                print("run %d %-11s: device %.3f ms = projection %.3f + ring pass %.3f ms; call %.2f ms wall" % (r, what, sum(s), s[0], s[2], 1e3 * wall))
            else:
                assert out[0].tobytes() == first[i][0].tobytes() and out[1].tobytes() == first[i][1].tobytes()
                print("run %d %-11s: device %.3f ms in %d launches; call %.2f ms wall, %.1f MB to the host"
                      % (r, what, s[2], int((ph["phase"] == 2).sum()), 1e3 * wall, 1e-6 * (out[0].nbytes + out[1].nbytes)))
    A, Ar = np.median(tot["A rings"]), np.median(ring)
    for what in ("B grouped", "B one group"):
        v = np.array(tot[what])
        B = np.median(v)
        print("%-11s: device time median %.3f ms, min %.3f, max %.3f over %d runs; B / A = %.3f (A = %.3f ms), B / A's ring pass "
              "= %.3f (%.3f ms); %.2f x the byte floor" % (what, B, v.min(), v.max(), len(v), B / A, A, B / Ar, Ar,
                                                         1e-3 * B / (must / COPY_RATE)))
    E.close()


if __name__ == "__main__":
    main()
