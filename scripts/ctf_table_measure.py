#!/usr/bin/env python3
"""What the CTF table (bioem_hip_enable_ctf_table: a second fold of every launch's partials, k_fold_ctf) costs a pass.
A = table off, B = table on, alternated A B A B on ONE handle of one box, for two shapes at 224^2, 5 CTF sets, +-10 px:
BASELINE config 2 (1 000 particles) and the 20-particle x 2 304-orientation job.  Per run: the comparison kernel's time
per launch from bioem_hip_kernel_stats (HIP events around the comparison kernel alone: the folds are NOT in it), the
comparison phase per launch from the phase records (the kernel and the folds behind it: the table's fold IS in it) and
the wall time per pass.  -> profiles/ctf_table_ab.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_run(E, W, on, passes):
    import bioem_amd.engine as eng
    E.enable_ctf_table(on)
    raw = eng.new_prob_block(W.nP, W.nOrient, 0)[0]
    walls, kern, phase, launches = [], [], [], 0
    for _ in range(passes):
        E.reset_kernel_stats()
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        E.start_run(raw)
        E.project_convolve_compare(0, W.nOrient)
        E.finish_run(raw)
        walls.append(1e3 * (time.perf_counter() - t0))
        ms, launches, _ = E.kernel_stats()
        rec = E.phase_records()
        E.set_phase_timing(False)
        kern.append(ms / launches)
        phase.append(1e3 * rec["seconds"][rec["phase"] == 2].sum() / launches)
    return dict(wall=float(np.median(walls)), kernel=float(np.median(kern)), phase=float(np.median(phase)),
                launches=int(launches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=224)
    ap.add_argument("--orientations", type=int, default=4608, help="of the 1 000-particle shape (config 2: 4 608)")
    ap.add_argument("--passes", type=int, default=3, help="passes per run; the median is reported")
    ap.add_argument("--alternations", type=int, default=2, help="A B pairs per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctf_table_ab.txt"))
    a = ap.parse_args()
    from bioem_amd.synthetic import Workload
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for nP, nO in ((1000, a.orientations), (20, 2304)):
        # noise particles: the time of a pass does not depend on what the images hold, and rendering 1 000 of them does
        W = Workload(N=a.pixels, nP=nP, nOrient=nO, nEnv=5, maxD=10, render=False)
        E = W.engine
        E.upload_particle_maps(np.random.default_rng(7).standard_normal((nP, a.pixels, a.pixels)).astype(np.float32))
        say("%d^2, %d particles x %d orientations x %d CTF sets, +-10 px, %s" % (a.pixels, nP, nO, W.nCTF, E.kernel_signature))
        one_run(E, W, False, 1)  # code load, buffers
        res = {False: [], True: []}
        for k in range(a.alternations):
            for on in (False, True):
                r = one_run(E, W, on, a.passes)
                res[on].append(r)
                say("  %s%d table %-3s: comparison kernel %.4f ms per launch, comparison phase with folds %.4f ms per launch "
                    "(%d launches), pass %.2f ms wall" % ("B" if on else "A", k, "on" if on else "off", r["kernel"], r["phase"],
                                                           r["launches"], r["wall"]))
        for key, what in (("kernel", "comparison kernel per launch"), ("phase", "comparison phase per launch"),
                          ("wall", "pass, wall")):
            av = [r[key] for r in res[False]]
            bv = [r[key] for r in res[True]]
            am, bm = float(np.mean(av)), float(np.mean(bv))
            say("  %s: A %.4f ms (runs differ by %.2f %%), B %.4f ms: B - A = %+.2f %%"
                % (what, am, 100.0 * (max(av) - min(av)) / am, bm, 100.0 * (bm - am) / am))
        E.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
