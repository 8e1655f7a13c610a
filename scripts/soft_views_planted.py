#!/usr/bin/env python3
"""Half-map Fourier shell correlation of the hard and the posterior-weighted reconstruction on a noisy planted set: the
synthetic model of bioem_amd/synthetic.py at 64^2, --particles particles rendered from random orientations of the run's
own list with a CTF set, a shift inside the window and noise at --snr, one run over all orientations, then
  hard      Engine.reconstruct of the arg-max records (--Reconstruct)
  soft K=1  Engine.reconstruct_soft over every CTF set and window cell at the arg-max orientation (--ReconstructSoft 1)
  soft K=3  ... at the three best orientations of the angle table (--ReconstructSoft 3)
each for the even and the odd particles.  A report: per shell the three FSC curves side by side, the resolutions read off
them and how far the posteriors are from one cell.  Nothing is asserted and no claim is made about which map is better.
-> profiles/soft_views_planted.txt"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=64)
    ap.add_argument("--particles", type=int, default=600)
    ap.add_argument("--orientations", type=int, default=300)
    ap.add_argument("--snr", type=float, default=0.05)
    ap.add_argument("--wiener", type=float, default=0.1)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd import reconstruct as rc, soft_views as sv, view_average as va
    from bioem_amd.synthetic import Workload
    N, nP, nO, K = a.pixels, a.particles, a.orientations, 3
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=3, maxD=4, npts=600, write_angles=K, render=False)
    E = W.engine
    E.upload_particle_maps(W.render_particles(a.snr, maxshift=3))
    raw, pmap, _ = eng.new_prob_block(nP, 0, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, nO)
    E.finish_run(raw)
    numconst = 0.5 * math.log(math.pi) + (1 - float(W.pd.Ntotpi) * 0.5) * (math.log(2 * math.pi) + 1) + math.log(float(W.pd.volu))
    cand = E.topk_angles(K, numconst)
    planted = (7919 * np.arange(nP)) % nO
    print("%d particles at %d^2, snr %g, %d orientations, %d CTF sets, window of %d x %d cells; the arg-max orientation is the "
          "planted one for %d particles, the planted one is among the best %d for %d"
          % (nP, N, a.snr, nO, W.nCTF, len(E.window_shifts()), len(E.window_shifts()), int((pmap["orient"] == planted).sum()), K,
             int((cand["orient"] == planted[:, None]).any(axis=1).sum())))
    halves = rc.half_weights(nP)
    g, orient = va.groups_by_orientation(pmap, 1, n_orient=nO)
    curves, res = {}, {}
    spec = [E.reconstruct(pmap, g, orient, w, wiener=a.wiener, want_spec=True, want_vol=False)["spec"] for w in halves]
    f, _, r05, r0143 = rc.derive(*rc.shell_sums(*spec)[1:], N, W.px)
    curves["hard"], res["hard"] = f, (r05, r0143)
    every = np.arange(nO, dtype=np.int32)
    for k in (1, K):
        spec = []
        for w in halves:
            mem, cells, req, pw = E.soft_members(pmap, K=k, topk=cand, weights=w, want_weights=True)
            spec.append(E.reconstruct_soft(mem, cells, every, wiener=a.wiener, want_spec=True, want_vol=False)["spec"])
        s = sv.particle_summary(req, pw, nP)
        f, _, r05, r0143 = rc.derive(*rc.shell_sums(*spec)[1:], N, W.px)
        curves["soft K=%d" % k], res["soft K=%d" % k] = f, (r05, r0143)
        print("soft K=%d: %d requests per particle; n_eff over (orientation, CTF set, cell): median %.3g, 90th percentile %.3g; mass on "
              "the arg-max cell: median %.3g, 10th percentile %.3g" % (k, int(s["requests"].max()), np.median(s["n_eff"]),
                                                                        np.percentile(s["n_eff"], 90), np.median(s["mass_argmax"]),
                                                                        np.percentile(s["mass_argmax"], 10)))
    names = list(curves)
    size = float(N) * float(W.px)
    print("shell resolution[A] " + " ".join("FSC(%s)" % n for n in names))
    for sh in range(1, N // 2 + 1):
        print("%5d %13.3f " % (sh, size / sh) + " ".join("%*.4f" % (len(n) + 5, curves[n][sh]) for n in names))
    for n in names:
        print("%-8s: resolution[A] at FSC < 0.5: %.3f, at FSC < 0.143: %.3f (-1: never below)" % (n, res[n][0], res[n][1]))
    E.close()


if __name__ == "__main__":
    main()
