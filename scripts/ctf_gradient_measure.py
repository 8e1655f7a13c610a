#!/usr/bin/env python3
"""Device time of the CTF gradient and curvature against the only way to the same numbers before it: the same 1 000 best
records at 224^2, batches of 64 records, from the engine's own phase records (HIP events on the stream).

 A7   the gradient by central differences: per record its triple and the six triples theta +- h e_t, log P of the seven
      through bioem_hip_ctf_scan; the records are grouped by their CTF set (a scan takes one candidate list), one call per
      set.  The candidates' kernels are built on the host (hostlib.ctf_kernel_list); that time is wall time, reported apart
 A19  the same with the twelve triples theta +- h e_t +- h e_u on top: the 3 x 3 Hessian by differences
 B    bioem_hip_ctf_gradient: the front half it shares with the other gradient entries (phases 0 and 1: projection, the
      scan's preparation and the linearisation) and the gradient pass (phases 2 and 3: k_ctfgrad_partials, k_ctfgrad_fold,
      k_ctfgrad_finish)

One handle on one device, A7, A19 and B alternating, the median of --repeats runs; the first call of each (staging buffers,
code load) is not counted.  The particles are noise images (no call depends on what they hold), the records drawn here.  No
target is set.
-> profiles/ctf_gradient_measure.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def candidates(theta, h, pairs):
    """the triple, its six neighbours and, with pairs, the twelve diagonal ones: float32 [7 or 19, 3]"""
    out = [np.array(theta, dtype=np.float64)]
    for t in range(3):
        for s in (1.0, -1.0):
            v = np.array(theta, dtype=np.float64)
            v[t] += s * h[t]
            out.append(v)
    for t in range(3):
        for u in range(t + 1, 3):
            for s1 in (1.0, -1.0):
                for s2 in (1.0, -1.0):
                    v = np.array(theta, dtype=np.float64)
                    v[t] += s1 * h[t]
                    v[u] += s2 * h[u]
                    if pairs:
                        out.append(v)
    return np.array(out, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=224)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--orientations", type=int, default=4608)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
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
    h = (0.004, 0.5, 1.0)
    groups = []
    for c in range(W.nCTF):
        idx = np.flatnonzero(pmap["conv"] == c)
        scan = np.zeros(len(idx), dtype=eng.SCAN_REQUEST_DTYPE)
        scan["particle"], scan["orient"] = idx, pmap["orient"][idx]
        scan["shiftX"], scan["shiftY"] = pmap["cent_x"][idx], pmap["cent_y"][idx]
        groups.append(scan)
    print("%d records at %d^2, %d CTF sets, batches of %d records; h = %s" % (nP, N, W.nCTF, E.max_batch()[0], h), flush=True)

    def timed(call):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        ph = E.phase_records()
        E.set_phase_timing(False)
        return out, ph, 1e3 * wall

    host_ms = {}

    def run_a(pairs):
        t = 0.0
        for c, scan in enumerate(groups):
            if not len(scan):
                continue
            cand = candidates(W.ctfParam[c], h, pairs)
            t0 = time.perf_counter()
            kern = hostlib.ctf_kernel_list(N, W.px, cand)
            t += time.perf_counter() - t0
            E.ctf_scan(scan, kern, cand)
        host_ms[pairs] = 1e3 * t

    run_b = lambda: E.best_match_ctf_gradient(pmap, W.px)  # noqa: E731
    run_a(False)
    run_a(True)
    ref = run_b()["rows"].tobytes()       # (the first calls: staging)
    tot = {"A7": [], "A19": [], "B": [], "Bf": [], "Bp": []}
    for r in range(a.repeats):
        for name, pairs in (("A7", False), ("A19", True)):
            _, ph, wall = timed(lambda: run_a(pairs))
            s = [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(4)]
            tot[name].append(sum(s))
            print("run %d %s: device %.2f ms = projection %.2f + preparation %.2f + scan %.2f; kernels built on the host %.1f ms; "
                  "calls %.1f ms wall" % (r, name, sum(s), s[0], s[1], s[2], host_ms[pairs], wall), flush=True)
        out, ph, wall = timed(run_b)
        assert out["rows"].tobytes() == ref
        front, pass_ = 1e3 * ph["seconds"][ph["phase"] < 2].sum(), 1e3 * ph["seconds"][ph["phase"] >= 2].sum()
        tot["B"].append(front + pass_)
        tot["Bf"].append(front)
        tot["Bp"].append(pass_)
        print("run %d B: device %.2f ms = front half %.2f + gradient pass %.2f; call %.1f ms wall" % (r, front + pass_, front, pass_, wall),
              flush=True)
    med = {k: float(np.median(v)) for k, v in tot.items()}
    print("medians over %d runs: A7 %.2f ms; A19 %.2f ms; B %.2f ms = front half %.2f + gradient pass %.2f; A7 / B = %.2f, A19 / B "
          "= %.2f" % (a.repeats, med["A7"], med["A19"], med["B"], med["Bf"], med["Bp"], med["A7"] / med["B"], med["A19"] / med["B"]),
          flush=True)
    E.close()


if __name__ == "__main__":
    main()
