#!/usr/bin/env python3
"""Device time of bioem_hip_window_posterior against bioem_hip_render_best_maps over the same records on the config-2
workload (224^2, 1 000 particles, 4 608 orientations, 5 CTFs, +-10 px): the engine's own phase records (HIP events on
the stream; window: 0 projection, 1 conv and the ordered Parseval sums, 2 the particle spectra's way back to reference
layout, column pass and cell pass; render: 0 projection, 1 column pass, 2 row pass) and the wall time of the calls,
copies to the host included.  One process, one device, the two calls alternating; the first call of each (staging
buffers, code load) is not counted.  The particles are noise images (the pass does not depend on what they hold), the
records drawn here.  The render is the yardstick because it is a double-precision DFT over the same inputs that keeps
all N rows where the window pass keeps nd.  -> profiles/best_window_measure.txt"""
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
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=a.pixels, nP=a.particles, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    rng = np.random.default_rng(1)
    E.upload_particle_maps(rng.standard_normal((a.particles, a.pixels, a.pixels)).astype(np.float32))
    rec = np.zeros(a.particles, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"] = rng.integers(0, a.orientations, a.particles)
    rec["conv"] = rng.integers(0, W.nCTF, a.particles)
    rec["cent_x"] = rng.integers(-10, 11, a.particles)
    rec["cent_y"] = rng.integers(-10, 11, a.particles)
    rec["norm"], rec["mu"] = 0.01, -0.02
    nd = len(E.window_shifts())
    print("%d records at %d^2, %d orientations x %d CTFs on the handle, batches of %d, %d x %d cells"
          % (a.particles, a.pixels, a.orientations, W.nCTF, E.max_batch()[0], nd, nd))
    first = E.best_match_window(rec)  # first calls: staging buffers, code load
    E.render_best_maps(rec)
    tot = {"window": [], "render": []}
    for r in range(a.repeats):
        for what, call in (("window", E.best_match_window), ("render", E.render_best_maps)):
            E.set_phase_timing(True)
            t0 = time.perf_counter()
            out = call(rec)
            wall = time.perf_counter() - t0
            ph = E.phase_records()
            E.set_phase_timing(False)
            s = [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(3)]
            tot[what].append(sum(s))
            if what == "window":
                assert out.tobytes() == first.tobytes()
                print("run %d window: device %.2f ms = projection %.2f + conv and sums %.2f + window pass %.2f ms (%d batches); "
                      "call %.2f ms wall, %.2f MB to the host; %.2f us per record on the device"
                      % (r, sum(s), s[0], s[1], s[2], int((ph["phase"] == 0).sum()), 1e3 * wall, 1e-6 * out.nbytes,
                         1e3 * sum(s) / a.particles))
            else:
                print("run %d render: device %.2f ms = projection %.2f + column pass %.2f + row pass %.2f ms; call %.2f ms "
                      "wall, %.0f MB to the host" % (r, sum(s), s[0], s[1], s[2], 1e3 * wall, 1e-6 * out.nbytes))
    for what in ("window", "render"):
        v = np.array(tot[what])
        print("%-6s: device time median %.2f ms, min %.2f, max %.2f over %d runs" % (what, np.median(v), v.min(), v.max(), len(v)))
    print("window / render (medians): %.3f" % (np.median(tot["window"]) / np.median(tot["render"])))
    E.close()


if __name__ == "__main__":
    main()
