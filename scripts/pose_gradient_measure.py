#!/usr/bin/env python3
"""Device time of the pose gradient of a volume model against the only way to the same six numbers before it: the same
1 000 best records at 224^2, batches of 64 records, from the engine's own phase records (HIP events on the stream).

 A  central differences: per record six orientations, the seed turned by +-h about each axis of the image frame
    (pose_gradient.step), uploaded as the particle's own list, and log P of the six through the own-list bioem_hip_ctf_scan
    against the handle's CTF sets (every phase of the scan; the upload of the lists is not counted)
 B  bioem_hip_pose_gradient: the front half it shares with bioem_hip_volume_gradient (phases 0, 1 and 2: projection as
    slices, the scan's preparation and the linearisation, the gradient spectrum and Y) and the pose pass (phase 3:
    k_pose_partials and k_pose_fold)

One handle on one device, A and B alternating, the median of --repeats runs; the first call of each (staging buffers, code
load) is not counted.  The particles are noise images (no call depends on what they hold), the records drawn here, the
volume a random positive blob.  No target is set.
-> profiles/pose_gradient_measure.txt"""
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
    ap.add_argument("--step", type=float, default=0.004)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd import pose_gradient as pose
    from bioem_amd.synthetic import Workload
    N, nP = a.pixels, a.particles
    W = Workload(N=N, nP=nP, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    rng = np.random.default_rng(1)
    E.upload_particle_maps(rng.standard_normal((nP, N, N)).astype(np.float32))
    pmap = np.zeros(nP, dtype=eng.PROB_MAP_DTYPE)
    pmap["orient"] = rng.integers(0, a.orientations, nP)
    pmap["conv"] = rng.integers(0, W.nCTF, nP)
    pmap["cent_x"], pmap["cent_y"] = rng.integers(-10, 11, nP), rng.integers(-10, 11, nP)
    pmap["norm"], pmap["mu"] = 1.0, 0.0
    x = np.arange(N) - (N + 1) // 2
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    vol = (rng.uniform(0.1, 1.0, (N, N, N)) * (r2 <= (N / 5.0) ** 2)).astype(np.float32)
    turns = [s * a.step * np.eye(3)[d] for d in range(3) for s in (1.0, -1.0)]
    lists = np.array([[pose.step(W.angles[o], w) for w in turns] for o in pmap["orient"]], dtype=np.float32)
    E.upload_particle_orientation_lists((lists.reshape(-1, 4), 6 * np.arange(nP + 1, dtype=np.int64)), True)
    scan = np.zeros(6 * nP, dtype=eng.SCAN_REQUEST_DTYPE)
    scan["particle"] = np.repeat(np.arange(nP), 6)
    scan["orient"] = np.tile(np.arange(6), nP)
    scan["shiftX"], scan["shiftY"] = np.repeat(pmap["cent_x"], 6), np.repeat(pmap["cent_y"], 6)
    print("%d records at %d^2, %d CTF sets, batches of %d records; A: %d requests of the own-list scan, h = %g"
          % (nP, N, W.nCTF, E.max_batch()[0], len(scan), a.step), flush=True)

    def timed(call):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        ph = E.phase_records()
        E.set_phase_timing(False)
        return out, ph, 1e3 * wall

    run_a = lambda: E.ctf_scan(scan, W.refCTF, W.ctfParam, own=True)  # noqa: E731
    run_b = lambda: E.best_match_pose_gradient(pmap)  # noqa: E731
    for pad in a.pads:
        E.upload_model_volume(vol, pad=pad)
        run_a()
        ref = run_b()["pose"].tobytes()       # (the first calls: staging)
        tot = {"A": [], "B": [], "Bf": [], "Bp": []}
        for r in range(a.repeats):
            _, ph, wall = timed(run_a)
            s = [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(4)]
            tot["A"].append(sum(s))
            print("pad %d run %d A: device %.2f ms = projection %.2f + preparation %.2f + scan %.2f + fold %.2f; call %.1f ms "
                  "wall" % (pad, r, sum(s), s[0], s[1], s[2], s[3], wall), flush=True)
            out, ph, wall = timed(run_b)
            assert out["pose"].tobytes() == ref
            front, pass_ = 1e3 * ph["seconds"][ph["phase"] < 3].sum(), 1e3 * ph["seconds"][ph["phase"] == 3].sum()
            tot["B"].append(front + pass_)
            tot["Bf"].append(front)
            tot["Bp"].append(pass_)
            print("pad %d run %d B: device %.2f ms = front half %.2f + pose pass %.2f; call %.1f ms wall"
                  % (pad, r, front + pass_, front, pass_, wall), flush=True)
        med = {k: float(np.median(v)) for k, v in tot.items()}
        print("pad %d medians over %d runs: A %.2f ms; B %.2f ms = front half %.2f + pose pass %.2f; A / B = %.2f"
              % (pad, a.repeats, med["A"], med["B"], med["Bf"], med["Bp"], med["A"] / med["B"]), flush=True)
    E.close()


if __name__ == "__main__":
    main()
