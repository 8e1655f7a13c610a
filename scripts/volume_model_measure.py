#!/usr/bin/env python3
"""Device time of the slice pass of a volume model (k_recon_matrices + k_slice_project, phase 0 of a run) against what it
replaces, from the engine's own phase records (HIP events on the stream); one process, one device, one build, the handles
alternating, the first run of each not counted, medians over --repeats runs.
(a) 224^2, one batch of 64 orientations: the slice pass at pad 1 and 2 against projection + r2c of the 2 000-point model of
    BASELINE config 2;
(b) 64^2: the slice pass against the projection of the same volume read as --ReadModelMRC reads it (262 144 points of
    radius 2 px), the only way before;
(c) a config-2 run (224^2, 1 000 particles, 4 608 orientations, 5 CTFs) with the volume model (pad 2) against the point
    model: comparisons per second of wall time.
The particles are noise images and the volume is the point model binned to voxels: the passes do not depend on what they
hold.  -> profiles/volume_model_measure.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def binned(points, px, N):
    """the point model as a density on the voxel grid, origin at voxel (N + 1) // 2"""
    o = (N + 1) // 2
    idx = np.clip(np.rint(points["pos"].astype(np.float64) / float(px)).astype(np.int64) + o, 0, N - 1)
    vol = np.zeros((N, N, N), dtype=np.float32)
    np.add.at(vol, (idx[:, 0], idx[:, 1], idx[:, 2]), points["density"])
    return vol


def phase0(E, run):
    E.set_phase_timing(True)
    t0 = time.perf_counter()
    run(E)
    wall = time.perf_counter() - t0
    ph = E.phase_records()
    E.set_phase_timing(False)
    sec = ph["seconds"][ph["phase"] == 0]
    return 1e3 * float(sec.sum()), int(len(sec)), wall


def full_run(E):
    import bioem_amd.engine as eng
    raw = eng.new_prob_block(E.nMaps, E.nAngles, 0)[0]
    E.start_run(raw)
    E.project_convolve_compare(0, E.nAngles)
    E.finish_run(raw)


def alternate(handles, repeats, what):
    for _, E in handles:
        phase0(E, full_run)
    t = {k: [] for k, _ in handles}
    for r in range(repeats):
        for k, E in handles:
            ms, nb, wall = phase0(E, full_run)
            t[k].append((ms / nb, wall))
            print("%s, run %d, %-28s: phase 0 %.4f ms per batch (%d batches), run %.1f ms wall" % (what, r, k, ms / nb, nb, 1e3 * wall))
    return {k: np.median(np.array(v), axis=0) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-config2", action="store_true")
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    rng = np.random.default_rng(1)

    def handle(W, nP, nO, maps, model):
        E = eng.Engine(W.pd, nP, nO, W.nCTF, algo=1, device=0)
        E.upload_ctf(W.refCTF, W.ctfParam)
        E.upload_orientations(W.angles[:nO], True)
        E.upload_particle_maps(maps)
        t0 = time.perf_counter()
        model(E)
        return E, time.perf_counter() - t0

    # (a) 224^2
    N, nP, nO = 224, 16, 64
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=5, maxD=10, render=False)
    W.engine.close()
    vol = binned(W.points, W.px, N)
    maps = rng.standard_normal((nP, N, N)).astype(np.float32)
    hs = []
    for k, model in (("points (2 000)", lambda E: E.upload_model(W.points, W.NormDen, W.px)),
                     ("volume pad 1", lambda E: E.upload_model_volume(vol, pad=1)),
                     ("volume pad 2", lambda E: E.upload_model_volume(vol, pad=2))):
        E, up = handle(W, nP, nO, maps, model)
        print("(a) %d^2 %-16s: model upload %.2f s wall, batches of %d orientations" % (N, k, up, E.max_batch()[0]))
        hs.append((k, E))
    m = alternate(hs, a.repeats, "(a) %d^2" % N)
    for k, _ in hs:
        print("(a) %d^2 %-16s: median phase 0 %.4f ms per batch = %.2f of the point model's projection + r2c"
              % (N, k, m[k][0], m[k][0] / m["points (2 000)"][0]))
    for _, E in hs:
        E.close()

    # (b) 64^2: the volume as --ReadModelMRC reads it
    N, nP, nO = 64, 16, 128
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=5, maxD=5, render=False)
    W.engine.close()
    vol = binned(W.points, W.px, N) + np.float32(1e-3)
    maps = rng.standard_normal((nP, N, N)).astype(np.float32)
    pts = np.zeros(N ** 3, dtype=eng.POINT_DTYPE)
    g = (np.arange(N) + 1 - N / 2.0) * float(W.px)
    pts["pos"] = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    pts["radius"] = np.float32(2.0 * float(W.px))
    pts["density"] = np.roll(vol, (-1, -1, -1), axis=(0, 1, 2)).reshape(-1)
    hs = []
    for k, model in (("points (%d, radius 2 px)" % len(pts), lambda E: E.upload_model(pts, float(vol.sum()), W.px)),
                     ("volume pad 1", lambda E: E.upload_model_volume(vol, pad=1)),
                     ("volume pad 2", lambda E: E.upload_model_volume(vol, pad=2))):
        E, up = handle(W, nP, nO, maps, model)
        print("(b) %d^2 %-28s: model upload %.2f s wall, batches of %d orientations" % (N, k, up, E.max_batch()[0]))
        hs.append((k, E))
    m = alternate(hs, a.repeats, "(b) %d^2" % N)
    for k, _ in hs:
        print("(b) %d^2 %-28s: median phase 0 %.4f ms per batch" % (N, k, m[k][0]))
    for _, E in hs:
        E.close()

    # (c) config 2
    if not a.skip_config2:
        N, nP, nO = 224, 1000, 4608
        W = Workload(N=N, nP=nP, nOrient=nO, nEnv=5, maxD=10, render=False)
        W.engine.close()
        vol = binned(W.points, W.px, N)
        maps = rng.standard_normal((nP, N, N)).astype(np.float32)
        hs = []
        for k, model in (("points (2 000)", lambda E: E.upload_model(W.points, W.NormDen, W.px)),
                         ("volume pad 2", lambda E: E.upload_model_volume(vol, pad=2))):
            hs.append((k, handle(W, nP, nO, maps, model)[0]))
        m = alternate(hs, a.repeats, "(c) config 2")
        for k, _ in hs:
            print("(c) config 2 %-16s: median run %.1f ms wall, %.1f M comparisons/s; phase 0 %.4f ms per batch"
                  % (k, 1e3 * m[k][1], 1e-6 * nP * nO * W.nCTF / m[k][1], m[k][0]))
        for _, E in hs:
            E.close()


if __name__ == "__main__":
    main()
