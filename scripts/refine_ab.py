#!/usr/bin/env python3
"""Round 2 of the manual's refinement (one orientation list per particle), two ways, on one box:

  A  the only way without the own-list pass: a loop over the particles in ONE process on ONE reused handle of
     nMaps = 1 -- per particle: upload its spectrum, upload its list, start_run, fused entry, finish_run.  (Generous to
     the old way, which is a process, a model read and a particle transform per image.)
  B  bioem_hip_upload_particle_orientations + bioem_hip_compare_own_orientations, one handle.

    python scripts/refine_ab.py --mode B --pixels 224 --particles 1000 --entries 125      one JSON line
    python scripts/refine_ab.py --ab <parent build's libbioem_hip.so>                      A B A B per shape, a table
    python scripts/refine_ab.py --own-ab <parent build's libbioem_hip.so>                  the own-list pass itself, below

--own-ab compares the own-list pass of two builds: A = the parent's library (one comparison launch per particle), B = this
tree with one launch per batch where the shape runs k_compare_fast (--launch batch; opt-in), A B A B per shape, then the tree once more with the block
table in plain row order (R, --launch rows) -- the order of the table is a measured choice.  The parent has no lists of
different lengths: for the ragged shape A is this tree with one launch per particle (--launch particle).  The last column says
whether B is slower than A beyond the spread of A's own two runs.  After the shapes, two alternations of
`bench.py --config 2` on the parent's library and on the tree's: the all-to-all path's sanity line.  --only 0,1,4 keeps
to those entries of the shape list (10 = the bench.py line), so that a run fits a time limit.

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
# (pixels, particles, entries; entries 0: the ragged mix, lengths 1 ... 125)
OWN_SHAPES = [(224, 20, 125), (224, 1000, 125), (128, 20, 125), (128, 1000, 125), (224, 1000, 27), (224, 1000, 5),
              (128, 1000, 27), (128, 1000, 5), (128, 10000, 27), (224, 1000, 0)]


def one(args):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload, random_quaternions
    N, nP, K = args.pixels, args.particles, args.entries
    lengths = None
    if K == 0:  # the ragged mix: lengths 1 ... 125, every length as often as the others
        lengths = 1 + (37 * np.arange(nP)) % 125
        K = 125
    W = Workload(N=N, nP=nP if args.mode == "B" else 1, nOrient=K, nEnv=args.envelopes, render=False)
    rng = np.random.default_rng(7)
    lists = random_quaternions(nP * K, 11).reshape(nP, K, 4)
    nRows = nP * K
    if lengths is not None:
        assert args.mode == "B"
        offsets = np.zeros(nP + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lengths)
        nRows = int(offsets[-1])
        ragged = (np.ascontiguousarray(lists.reshape(-1, 4)[:nRows]), offsets)
    E = W.engine
    if args.launch:
        E.set_own_launch(args.launch)
    times = []
    if args.mode == "B":
        E.upload_particle_maps(rng.normal(size=(nP, N, N)).astype(np.float32))
        raw = eng.new_prob_block(nP, K, 0)[0]
        for it in range(args.reps + 1):
            raw[:] = eng.new_prob_block(nP, K, 0)[0]
            t0 = time.perf_counter()
            if lengths is None:
                E.upload_particle_orientations(lists, True)
            else:
                E.upload_particle_orientation_lists(ragged, True)
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
    own = E.own_kernel_signature if hasattr(E.L, "bioem_hip_own_kernel_signature") else "per particle: " + E.kernel_signature
    print(json.dumps({"mode": args.mode, "pixels": N, "particles": nP, "entries": args.entries, "ctfs": W.nCTF,
                      "kernel": E.kernel_signature, "own": own if args.mode == "B" else "", "seconds_per_pass": t,
                      "passes": [round(x, 6) for x in times[1:]], "comparisons_per_s": nRows * W.nCTF / t}))
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


def own_ab(args):
    print("# own-list pass, %d CTFs: A = the parent's build (one comparison launch per particle), B = this tree, --launch batch (one launch per"
          % args.envelopes)
    print("# batch: k_compare_fast_own, block table with a particle's blocks on one XCD), R = this tree, table in row order;")
    print("# A B A B R, every run a process of its own; median of %d passes after a warm-up; ragged: lengths 1 ... 125, A = this"
          % args.reps)
    print("# tree with --launch particle")
    only = [int(x) for x in args.only.split(",")] if args.only else list(range(len(OWN_SHAPES) + 1))
    for i, (N, nP, K) in enumerate(OWN_SHAPES):
        if i not in only:
            continue
        res = {"A": [], "B": [], "R": []}
        what = "%d^2 x %5d particles x %s entries" % (N, nP, "1..125" if K == 0 else "%3d" % K)
        for mode in ("A", "B", "A", "B", "R"):
            env = dict(os.environ)
            env.pop("BIOEM_HIP_LIBRARY", None)
            launch = []
            if mode == "A" and K != 0:
                env["BIOEM_HIP_LIBRARY"] = os.path.abspath(args.own_ab)
            elif mode == "A":
                launch = ["--launch", "particle"]
            elif mode == "R":
                launch = ["--launch", "rows"]
            elif mode == "B":
                launch = ["--launch", "batch"]
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "B", "--pixels", str(N), "--particles",
                                str(nP), "--entries", str(K), "--envelopes", str(args.envelopes), "--reps", str(args.reps)]
                               + launch, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:])
                sys.exit("refine_ab: %s at %s failed (exit %d): stopping" % (mode, what, r.returncode))
            d = json.loads(r.stdout.strip().split("\n")[-1])
            res[mode].append(d)
            print("%s  %s: %9.3f ms per pass  %7.3f M comparisons/s  (%s)"
                  % (what, mode, 1e3 * d["seconds_per_pass"], d["comparisons_per_s"] / 1e6, d["own"]), flush=True)
        ta = [d["seconds_per_pass"] for d in res["A"]]
        tb = [d["seconds_per_pass"] for d in res["B"]]
        a, b, spread = float(np.mean(ta)), float(np.mean(tb)), abs(ta[0] - ta[1])
        print("%s  A / B = %.3f   A-to-A spread %.3f ms   rows / xcd = %.3f   %s"
              % (what, a / b, 1e3 * spread, res["R"][0]["seconds_per_pass"] / b,
                 "B slower beyond the spread" if b > a + spread else "B not slower"), flush=True)
    if len(OWN_SHAPES) in only:
        bench_ab(args)


def bench_ab(args):
    """the all-to-all path: bench.py --config 2, parent's library and the tree's, A B A B"""
    ms = {"A": [], "B": []}
    for mode in ("A", "B", "A", "B"):
        env = dict(os.environ)
        env.pop("BIOEM_HIP_LIBRARY", None)
        if mode == "A":
            env["BIOEM_HIP_LIBRARY"] = os.path.abspath(args.own_ab)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--steps", "5",
                            "--warmup", "2"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=args.timeout)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            sys.exit("refine_ab: bench.py --config 2, %s failed (exit %d): stopping" % (mode, r.returncode))
        d = json.loads(r.stdout.strip().split("\n")[-1])
        ms[mode].append(d["ms_per_step"])
        print("bench.py --config 2 --steps 5 --warmup 2  %s: %8.2f ms per step  %7.2f M comparisons/s"
              % (mode, d["ms_per_step"], d["value"] / 1e6), flush=True)
    print("bench.py --config 2  A %s  B %s  mean B / mean A = %.4f   A-to-A spread %.2f ms"
          % (" ".join("%.2f" % x for x in ms["A"]), " ".join("%.2f" % x for x in ms["B"]),
             np.mean(ms["B"]) / np.mean(ms["A"]), abs(ms["A"][0] - ms["A"][1])), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=["A", "B"])
    ap.add_argument("--ab", metavar="PARENT_LIB")
    ap.add_argument("--own-ab", metavar="PARENT_LIB")
    ap.add_argument("--only", metavar="I,J,...", help="--own-ab: these entries of the shape list only")
    ap.add_argument("--launch", choices=["batch", "rows", "particle"], help="mode B: Engine.set_own_launch")
    ap.add_argument("--pixels", type=int, default=224)
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--entries", type=int, default=125)
    ap.add_argument("--envelopes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.own_ab:
        own_ab(args)
    elif args.ab:
        ab(args)
    elif args.mode:
        one(args)
    else:
        ap.error("--mode A|B, --ab <library> or --own-ab <library>")


if __name__ == "__main__":
    main()
