#!/usr/bin/env python3
"""Round 2 of the manual's refinement (one orientation list per particle), two ways, on one box:

  A  the only way without the own-list pass: a loop over the particles in ONE process on ONE reused handle of
     nMaps = 1 -- per particle: upload its spectrum, upload its list, start_run, fused entry, finish_run.  (Generous to
     the old way, which is a process, a model read and a particle transform per image.)
  B  bioem_hip_upload_particle_orientations + bioem_hip_compare_own_orientations, one handle.

    python scripts/refine_ab.py --mode B --pixels 224 --particles 1000 --entries 125      one JSON line
    python scripts/refine_ab.py --ab <parent build's libbioem_hip.so>                      A B A B per shape, a table

--ab runs every (mode, shape) in a process of its own, A on the given library (BIOEM_HIP_LIBRARY), B on the tree's, each
under its own time limit; the first failure ends the run.  Host clock around work that ends in finish_run, one warm-up
pass, median of the timed passes.  Particles are noise and the lists random: the time does not depend on either."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(224, 20), (224, 1000), (128, 20), (128, 1000)]


def one(args):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload, random_quaternions
    N, nP, K = args.pixels, args.particles, args.entries
    W = Workload(N=N, nP=nP if args.mode == "B" else 1, nOrient=K, nEnv=args.envelopes, render=False)
    rng = np.random.default_rng(7)
    lists = random_quaternions(nP * K, 11).reshape(nP, K, 4)
    E = W.engine
    times = []
    if args.mode == "B":
        E.upload_particle_maps(rng.normal(size=(nP, N, N)).astype(np.float32))
        raw = eng.new_prob_block(nP, K, 0)[0]
        for it in range(args.reps + 1):
            raw[:] = eng.new_prob_block(nP, K, 0)[0]
            t0 = time.perf_counter()
            E.upload_particle_orientations(lists, True)
            E.start_run(raw)
            E.compare_own_orientations(0, nP)
            E.finish_run(raw)
            times.append(time.perf_counter() - t0)
    else:
        # the particles' spectra and sums, as PreCalculateMapsFFT leaves them: transformed once, outside the clock
        H = N // 2 + 1
        spec = np.empty((nP, N, H, 2), dtype=np.float32)
        s1 = np.empty(nP, dtype=np.float32)
        s2 = np.empty(nP, dtype=np.float32)
        for p in range(nP):
            E.upload_particle_maps(rng.normal(size=(1, N, N)).astype(np.float32))
            a, b, c = E.debug_particles()
            spec[p], s1[p], s2[p] = a[0], b[0], c[0]
        raw = eng.new_prob_block(1, K, 0)[0]
        fresh = raw.copy()
        for it in range(args.reps + 1):
            t0 = time.perf_counter()
            for p in range(nP):
                raw[:] = fresh
                E.upload_particles(spec[p:p + 1], s1[p:p + 1], s2[p:p + 1])
                E.upload_orientations(lists[p], True)
                E.start_run(raw)
                E.project_convolve_compare(0, K)
                E.finish_run(raw)
            times.append(time.perf_counter() - t0)
    t = float(np.median(times[1:]))
    print(json.dumps({"mode": args.mode, "pixels": N, "particles": nP, "entries": K, "ctfs": W.nCTF, "kernel": E.kernel_signature,
                      "seconds_per_pass": t, "passes": [round(x, 6) for x in times[1:]],
                      "comparisons_per_s": nP * K * W.nCTF / t}))
    E.close()


def ab(args):
    print("# round 2, K = %d entries per particle, %d CTFs: A = loop over particles on a one-particle handle (the parent's build),"
          % (args.entries, args.envelopes))
    print("# B = own-list pass (this tree); A B A B, every run a process of its own; median of %d passes after a warm-up"
          % args.reps)
    for N, nP in SHAPES:
        res = {"A": [], "B": []}
        for mode in ("A", "B", "A", "B"):
            env = dict(os.environ)
            if mode == "A":
                env["BIOEM_HIP_LIBRARY"] = os.path.abspath(args.ab)
            else:
                env.pop("BIOEM_HIP_LIBRARY", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--pixels", str(N), "--particles",
                                str(nP), "--entries", str(args.entries), "--envelopes", str(args.envelopes), "--reps",
                                str(args.reps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               timeout=args.timeout)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:])
                sys.exit("refine_ab: %s at %d^2 x %d particles failed (exit %d): stopping" % (mode, N, nP, r.returncode))
            d = json.loads(r.stdout.strip().split("\n")[-1])
            res[mode].append(d)
            print("%d^2 x %4d particles  %s: %9.3f ms per pass  %7.3f M comparisons/s  (%s)"
                  % (N, nP, mode, 1e3 * d["seconds_per_pass"], d["comparisons_per_s"] / 1e6, d["kernel"]), flush=True)
        a = float(np.median([d["seconds_per_pass"] for d in res["A"]]))
        b = float(np.median([d["seconds_per_pass"] for d in res["B"]]))
        print("%d^2 x %4d particles  A / B = %.2f   B: %.3f M comparisons/s   %s"
              % (N, nP, a / b, nP * args.entries * res["B"][0]["ctfs"] / b / 1e6, "B faster" if b < a else "B NOT faster"),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=["A", "B"])
    ap.add_argument("--ab", metavar="PARENT_LIB")
    ap.add_argument("--pixels", type=int, default=224)
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--entries", type=int, default=125)
    ap.add_argument("--envelopes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.ab:
        ab(args)
    elif args.mode:
        one(args)
    else:
        ap.error("--mode A|B or --ab <library>")


if __name__ == "__main__":
    main()
