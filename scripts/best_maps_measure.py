#!/usr/bin/env python3
"""Device time of bioem_hip_render_best_maps on the config-2 workload (224^2, 1 000 particles, 4 608 orientations, 5 CTFs):
the engine's own phase records (HIP events on the stream: 0 projection, 1 column pass, 2 row pass per batch) and the wall
time of the call, copies to the host included.  No particles are needed: the records are drawn here (orientation and CTF
at random, shifts within +-10 px).  -> profiles/best_maps_render.txt"""
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
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=a.pixels, nP=a.particles, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    rng = np.random.default_rng(1)
    rec = np.zeros(a.particles, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"] = rng.integers(0, a.orientations, a.particles)
    rec["conv"] = rng.integers(0, W.nCTF, a.particles)
    rec["cent_x"] = rng.integers(-10, 11, a.particles)
    rec["cent_y"] = rng.integers(-10, 11, a.particles)
    rec["norm"], rec["mu"] = 0.01, -0.02
    print("render of %d records at %d^2, %d orientations x %d CTFs on the handle, batches of %d"
          % (a.particles, a.pixels, a.orientations, W.nCTF, E.max_batch()[0]))
    E.render_best_maps(rec)  # first call: staging buffers, code load
    for r in range(a.repeats):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        E.render_best_maps(rec)
        wall = time.perf_counter() - t0
        ph = E.phase_records()
        E.set_phase_timing(False)
        s = [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(3)]
        print("run %d: device %.2f ms = projection %.2f + column pass %.2f + row pass %.2f ms (%d batches); "
              "call %.2f ms wall, copies of %.0f MB to the host included; %.1f us per map on the device"
              % (r, sum(s), s[0], s[1], s[2], int((ph["phase"] == 0).sum()), 1e3 * wall,
                 4e-6 * a.particles * a.pixels ** 2, 1e3 * sum(s) / a.particles))
    E.close()


if __name__ == "__main__":
    main()
