#!/usr/bin/env python3
"""Device time of bioem_hip_view_sums_soft against bioem_hip_view_sums over the same particles on the config-2 workload
(224^2, 1 000 particles, 5 CTFs, +-10 px: tables of 21 x 21 cells, 50 views, batches of 64): the engine's own phase records
(HIP events on the stream).  A = view_sums (phase 2: the spectra's way back to reference layout and the accumulation);
B = view_sums_soft with one member per particle; C = with five members per particle, one per CTF set, in the particle's
view.  For B and C the three passes are recorded apart: phase 0 the column pass (U), phase 1 the row pass (W), phase 2
the spectra's way back and the accumulation.  One process, one device, the three calls alternating; the first call of
each (staging buffers, code load) is not counted; medians over --repeats runs.  The tables are random (the passes do not
depend on what they hold), the particles noise images.  Bytes: A reads the spectra once (8 B per coefficient and
particle); B writes and reads W as well (16 B each way per coefficient and member).
-> profiles/soft_views_measure.txt"""
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
    shifts = E.window_shifts()
    nd = len(shifts)

    def members(per):
        m = np.zeros(a.particles * per, dtype=eng.SOFT_MEMBER_DTYPE)
        m["particle"] = np.repeat(np.arange(a.particles), per)
        m["group"] = np.repeat(grouped, per)
        m["conv"] = (np.repeat(rec["conv"], per) + np.tile(np.arange(per), a.particles)) % W.nCTF
        m["s2"], m["b"], m["mass"] = 1e-4 / per, -2e-4 / per, 1.0 / per
        cells = rng.random((len(m), nd, nd))
        return m, cells * (0.01 / per / cells.sum(axis=(1, 2), keepdims=True))
    mB, cB = members(1)
    mC, cC = members(W.nCTF)
    M = a.pixels * (a.pixels // 2 + 1)
    must = 8.0 * M * a.particles
    print("%d particles at %d^2, %d CTFs on the handle, tables of %d x %d cells, batches of %d; %d views of %d..%d particles; the "
          "spectra are %.1f MB: %.3f ms at 6.3 TB/s; W of one member is %.2f MB"
          % (a.particles, a.pixels, W.nCTF, nd, nd, E.max_batch()[0], len(orient), np.bincount(grouped).min(),
             np.bincount(grouped).max(), 1e-6 * must, 1e3 * must / COPY_RATE, 16e-6 * M))
    calls = (("A view_sums", lambda: E.view_sums(rec, grouped)), ("B 1 member", lambda: E.view_sums_soft(mB, cB, shifts)),
             ("C %d members" % W.nCTF, lambda: E.view_sums_soft(mC, cC, shifts)))
    first = [c() for _, c in calls]  # first calls: staging buffers, code load
    tot = {k: [] for k, _ in calls}
    for r in range(a.repeats):
        for i, (what, call) in enumerate(calls):
            E.set_phase_timing(True)
            t0 = time.perf_counter()
            out = call()
            wall = time.perf_counter() - t0
            ph = E.phase_records()
            E.set_phase_timing(False)
            assert out[0].tobytes() == first[i][0].tobytes() and out[1].tobytes() == first[i][1].tobytes()
            s = [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(3)]
            tot[what].append(s)
            print("run %d %-11s: device %.3f ms = column pass %.3f + row pass %.3f + accumulation %.3f ms in %d launches; call "
                  "%.2f ms wall" % (r, what, sum(s), s[0], s[1], s[2], int((ph["phase"] == 2).sum()), 1e3 * wall))
    A = np.median([sum(s) for s in tot["A view_sums"]])
    for what, _ in calls:
        v = np.array(tot[what])
        t = v.sum(axis=1)
        print("%-11s: device time median %.3f ms, min %.3f, max %.3f over %d runs (column pass %.3f, row pass %.3f, accumulation "
              "%.3f ms); / A = %.3f; %.2f x A's byte floor"
              % (what, np.median(t), t.min(), t.max(), len(t), np.median(v[:, 0]), np.median(v[:, 1]), np.median(v[:, 2]),
                 np.median(t) / A, 1e-3 * np.median(t) / (must / COPY_RATE)))
    E.close()


if __name__ == "__main__":
    main()
