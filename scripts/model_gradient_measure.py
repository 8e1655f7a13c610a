#!/usr/bin/env python3
"""Device time of the density gradient against the best-map render on one handle: the same 1 000 best records at 224^2,
batches of 64 records, from the engine's own phase records (HIP events on the stream).

 A  bioem_hip_render_best_maps, the nearest existing call with the same passes (phases: 0 projection, 1 the column
    pass of the inverse transform with the convolution, 2 the row pass)
 B  bioem_hip_model_gradient without the rows (phases: 0 projection, 1 the scan's preparation per batch and the
    linearisation -- one CTF scan of up to 16 batches against the handle's own sets, then a, b, g --, 2 the gradient
    spectrum and the inverse transform, 3 the gather and the fold)

One process, one device, A and B alternating, the median of --repeats runs; the first call of each (staging buffers, code
load) is not counted.  The particles are noise images (neither call depends on what they hold), the records drawn here.
No target is set: the expectation is the render's cost plus a gather of the projection's order plus the linearisation.
-> profiles/model_gradient_measure.txt"""
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
    pmap = np.zeros(a.particles, dtype=eng.PROB_MAP_DTYPE)
    pmap["orient"] = rng.integers(0, a.orientations, a.particles)
    pmap["conv"] = rng.integers(0, W.nCTF, a.particles)
    pmap["cent_x"], pmap["cent_y"] = rng.integers(-10, 11, a.particles), rng.integers(-10, 11, a.particles)
    pmap["norm"], pmap["mu"] = 1.0, 0.0
    print("%d records at %d^2, %d model points, %d CTF sets, batches of %d records"
          % (a.particles, a.pixels, E._nPts, W.nCTF, E.max_batch()[0]))

    def timed(call, phases):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        ph = E.phase_records()
        E.set_phase_timing(False)
        return out, [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(phases)], 1e3 * wall

    run_a = lambda: E.render_best_maps(pmap)  # noqa: E731
    run_b = lambda: E.best_match_gradient(pmap, want_grad=False)  # noqa: E731
    first_a, first_b = run_a(), run_b()
    acc = first_b["points"]
    print("B: %d requests with coefficients that are not finite; |sum rho g| / sum |rho g| = %.3g"
          % (int((~np.isfinite(first_b["coef"][:, :3]).all(axis=1)).sum()),
             abs(float(np.dot(W.points["density"].astype(np.float64), acc["sum"])))
             / max(float(np.abs(W.points["density"].astype(np.float64) * acc["sum"]).sum()), 1e-300)))
    tot = {"A": [], "B": []}
    names = {"A": ("projection", "columns", "rows"),
             "B": ("projection", "preparation and linearisation", "spectrum and inverse", "gather and fold")}
    for r in range(a.repeats):
        for what, call in (("A", run_a), ("B", run_b)):
            out, s, wall = timed(call, len(names[what]))
            tot[what].append(sum(s))
            if what == "B":
                assert out["points"].tobytes() == acc.tobytes()
            print("run %d %s: device %.2f ms = %s; call %.1f ms wall" % (
                r, what, sum(s), " + ".join("%s %.2f" % (n, v) for n, v in zip(names[what], s)), wall))
    for what in ("A", "B"):
        v = np.array(tot[what])
        print("%s: device time median %.2f ms, min %.2f, max %.2f over %d runs" % (what, np.median(v), v.min(), v.max(), len(v)))
    print("B / A (medians): %.2f" % (np.median(tot["B"]) / np.median(tot["A"])))
    E.close()


if __name__ == "__main__":
    main()
