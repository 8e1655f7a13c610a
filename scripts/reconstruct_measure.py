#!/usr/bin/env python3
"""Device time of bioem_hip_reconstruct against bioem_hip_view_sums over the same records on the config-2 workload (224^2,
1 000 particles, 5 CTFs): the engine's own phase records (HIP events on the stream).  The chain's time splits into the view
accumulation (phase 2), the insertion of the chunks of views into the Fourier volume (phase 1), the estimate (phase 0,
iOrientBegin 0) and the inverse to the real-space volume (phase 0, iOrientBegin 1).  Two groupings: the records spread over
--views orientations, and one view per particle.  The insertion is measured with the brick cull and without it
(BIOEM_HIP_RECON_NO_CULL; same bits, asserted here).  The denominator is view_sums alone over the same records and
groups, the only other consumer of the same data.  One process, one device, the calls alternating; the first call of each
(staging buffers, code load) is not counted; medians over --repeats runs.  The particles are noise images (the passes do
not depend on what they hold), the records drawn here.
-> profiles/reconstruct_measure.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=224)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--orientations", type=int, default=4608)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=a.pixels, nP=a.particles, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    rng = np.random.default_rng(1)
    E.upload_particle_maps(rng.standard_normal((a.particles, a.pixels, a.pixels)).astype(np.float32))
    rec = np.zeros(a.particles, dtype=eng.PROB_MAP_DTYPE)
    rec["Total"] = 1.0
    rec["conv"] = rng.integers(0, W.nCTF, a.particles)
    rec["cent_x"] = rng.integers(-10, 11, a.particles)
    rec["cent_y"] = rng.integers(-10, 11, a.particles)
    rec["norm"], rec["mu"] = 0.01, -0.02
    N, H = a.pixels, a.pixels // 2 + 1
    print("%d records at %d^2, %d CTFs on the handle, batches and chunks of %d; the volume buffers take %.1f MB"
          % (a.particles, N, W.nCTF, E.max_batch()[0], 40e-6 * N * N * H))
    for label, nViews in (("%d views" % a.views, a.views), ("one view per particle", a.particles)):
        orient = np.sort(rng.choice(a.orientations, nViews, replace=False)).astype(np.int32)
        group = (np.arange(a.particles) % nViews).astype(np.int32) if nViews == a.particles else \
            rng.integers(0, nViews, a.particles).astype(np.int32)
        calls = (("sums", lambda: E.view_sums(rec, group, n_groups=nViews)),
                 ("chain", lambda: E.reconstruct(rec, group, orient)),
                 ("chain, no cull", lambda: E.reconstruct(rec, group, orient, cull=False)))
        first = [c() for _, c in calls]
        both = [E.reconstruct(rec, group, orient, want_spec=True, cull=c) for c in (True, False)]
        assert all(both[0][k].tobytes() == both[1][k].tobytes() for k in ("vol", "spec", "den"))
        assert first[1]["vol"].tobytes() == both[0]["vol"].tobytes()
        t = {k: [] for k, _ in calls}
        for r in range(a.repeats):
            for what, call in calls:
                E.set_phase_timing(True)
                t0 = time.perf_counter()
                call()
                wall = time.perf_counter() - t0
                ph = E.phase_records()
                E.set_phase_timing(False)
                p0 = ph["phase"] == 0
                sec = 1e3 * ph["seconds"]
                s = [sec[ph["phase"] == 2].sum(), sec[ph["phase"] == 1].sum(), sec[p0 & (ph["iOrientBegin"] == 0)].sum(),
                     sec[p0 & (ph["iOrientBegin"] == 1)].sum()]
                t[what].append(s)
                print("%s, run %d %-15s: device %.3f ms = accumulation %.3f + insertion %.3f + estimate %.3f + inverse %.3f; "
                      "call %.1f ms wall" % (label, r, what, sum(s), s[0], s[1], s[2], s[3], 1e3 * wall))
        m = {k: np.median(np.array(v), axis=0) for k, v in t.items()}
        B = m["sums"][0]
        for what in ("chain", "chain, no cull"):
            s = m[what]
            print("%s, %-15s: medians over %d runs: device %.3f ms = accumulation %.3f + insertion %.3f + estimate %.3f + "
                  "inverse %.3f; view_sums alone %.3f ms, chain / view_sums = %.2f"
                  % (label, what, a.repeats, s.sum(), s[0], s[1], s[2], s[3], B, s.sum() / B))
    E.close()


if __name__ == "__main__":
    main()
