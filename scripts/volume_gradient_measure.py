#!/usr/bin/env python3
"""Device time of the density gradient per voxel of a volume model against the gradient per point of a point model: the
same 1 000 best records at 224^2, batches of 64 records, from the engine's own phase records (HIP events on the stream).

 A  bioem_hip_model_gradient on the 2 000-point model without the rows (the parent's entry; phases of
    scripts/model_gradient_measure.py)
 B  bioem_hip_volume_gradient on a volume model at pad 1 and pad 2: the shared front half (phases 0, 1 and 2: projection
    as slices, the scan's preparation and the linearisation, the gradient spectrum with Y and <C, A_r>), the
    back-insertion (phase 3 per batch) and the passes back to the volume (the record of phase 3 with the empty request
    range [n, n); its events also span the entry's temporary allocations and the copy of the volume to the host)

Two handles in one process on one device, A and B alternating, the median of --repeats runs; the first call of each
(staging buffers, code load) is not counted.  The particles are noise images (no call depends on what they hold), the
records drawn here, the volume a random positive blob.  No target is set.
-> profiles/volume_gradient_measure.txt"""
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
    ap.add_argument("--pads", type=int, nargs="+", default=[1, 2])
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    N = a.pixels
    W = Workload(N=N, nP=a.particles, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    rng = np.random.default_rng(1)
    maps = rng.standard_normal((a.particles, N, N)).astype(np.float32)
    E.upload_particle_maps(maps)
    pmap = np.zeros(a.particles, dtype=eng.PROB_MAP_DTYPE)
    pmap["orient"] = rng.integers(0, a.orientations, a.particles)
    pmap["conv"] = rng.integers(0, W.nCTF, a.particles)
    pmap["cent_x"], pmap["cent_y"] = rng.integers(-10, 11, a.particles), rng.integers(-10, 11, a.particles)
    pmap["norm"], pmap["mu"] = 1.0, 0.0
    x = np.arange(N) - (N + 1) // 2
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    vol = (rng.uniform(0.1, 1.0, (N, N, N)) * (r2 <= (N / 5.0) ** 2)).astype(np.float32)
    print("%d records at %d^2, %d model points, %d CTF sets, batches of %d records"
          % (a.particles, N, E._nPts, W.nCTF, E.max_batch()[0]), flush=True)

    def timed(call):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        ph = E.phase_records()
        E.set_phase_timing(False)
        return out, ph, 1e3 * wall

    def split_a(ph):
        return [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(4)]

    def split_b(ph):
        passes = (ph["phase"] == 3) & (ph["iOrientBegin"] == ph["iOrientEnd"])
        front = 1e3 * ph["seconds"][ph["phase"] < 3].sum()
        return [front, 1e3 * ph["seconds"][(ph["phase"] == 3) & ~passes].sum(), 1e3 * ph["seconds"][passes].sum()]

    run_a = lambda: E.best_match_gradient(pmap, want_grad=False)  # noqa: E731
    run_b = lambda: E.best_match_volume_gradient(pmap)  # noqa: E731
    for pad in a.pads:
        E.upload_model(W.points, W.NormDen, W.px, 0, 0)
        run_a()
        tot = {"A": [], "B": [], "Bi": [], "Bp": [], "Bf": []}
        ref = None
        for r in range(a.repeats):
            E.upload_model(W.points, W.NormDen, W.px, 0, 0)
            _, ph, wall = timed(run_a)
            s = split_a(ph)
            tot["A"].append(sum(s))
            print("pad %d run %d A: device %.2f ms = projection %.2f + preparation and linearisation %.2f + spectrum and inverse "
                  "%.2f + gather and fold %.2f; call %.1f ms wall" % (pad, r, sum(s), s[0], s[1], s[2], s[3], wall), flush=True)
            E.upload_model_volume(vol, pad=pad)
            if ref is None:
                ref = run_b()["vol"].tobytes()       # (the first call: staging, A beside C)
            out, ph, wall = timed(run_b)
            assert out["vol"].tobytes() == ref
            s = split_b(ph)
            for k, v in zip(("Bf", "Bi", "Bp"), s):
                tot[k].append(v)
            tot["B"].append(sum(s))
            print("pad %d run %d B: device %.2f ms = front half %.2f + insert %.2f + passes back %.2f; call %.1f ms wall"
                  % (pad, r, sum(s), s[0], s[1], s[2], wall), flush=True)
        med = {k: float(np.median(v)) for k, v in tot.items()}
        print("pad %d medians over %d runs: A %.2f ms; B %.2f ms = front half %.2f + insert %.2f + passes back %.2f; B / A = %.2f"
              % (pad, a.repeats, med["A"], med["B"], med["Bf"], med["Bi"], med["Bp"], med["B"] / med["A"]), flush=True)
    E.close()


if __name__ == "__main__":
    main()
