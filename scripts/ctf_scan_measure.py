#!/usr/bin/env python3
"""Device time of a CTF scan two ways on one handle: 1 000 best records at 224^2 against 256 candidate CTF sets, batches
of 64 records, from the engine's own phase records (HIP events on the stream).

 A  the only way before bioem_hip_ctf_scan: the candidates become the handle's CTF sets, five at a time (the handle was
    created for five, which is what gives it batches of 64), and bioem_hip_window_posterior is called over every
    (record, candidate) at the handle's +-10 px window: nd^2 cells per pair where one is wanted, one sequential
    sumsquareC chain per pair (phases: 0 projection, 1 conv and the ordered Parseval sums, 2 the window pass)
 B  bioem_hip_ctf_scan over the same records and candidates (phases: 0 projection, 1 the preparation with the packing
    of the candidates, 2 the scan)

One process, one device, A and B alternating, the median of --repeats runs; the first call of each (staging buffers, code
load) is not counted.  The particles are noise images (neither pass depends on what they hold), the records drawn here.
B's results are held against A's at the records' cells: the same parameters bit for bit, log posteriors that differ by
the rounding of two summation orders at the most.

The records a wave of k_ctf_scan carries (R) is a compile-time constant of kernels_scan.hip: for another R build that
unit with -DBIOEM_SCAN_RECORDS=R into a library of its own and run this script again with BIOEM_HIP_LIBRARY=that library
and --skip-a.  -> profiles/ctf_scan_measure.txt"""
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
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-a", action="store_true", help="B alone (another build of the scan kernel)")
    ap.add_argument("--label", default="", help="printed with every line of B (which build this is)")
    a = ap.parse_args()
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
    from bioem_amd.synthetic import Workload
    W = Workload(N=a.pixels, nP=a.particles, nOrient=a.orientations, nEnv=5, maxD=10, render=False)
    E = W.engine
    nC = W.nCTF
    rng = np.random.default_rng(1)
    E.upload_particle_maps(rng.standard_normal((a.particles, a.pixels, a.pixels)).astype(np.float32))
    # the candidates: a defocus x envelope grid finer than the handle's
    G = a.candidates
    nPh = int(round(G ** 0.5))
    assert nPh * (G // nPh) == G, "a candidate count that factors into two axes"
    pha = np.linspace(W.ctfParam[:, 1].min() * 0.5 + 1.0, W.ctfParam[:, 1].max() * 2.0 + 2.0, nPh)
    env = np.linspace(2.0, 300.0, G // nPh)
    tr = np.array([(0.1, p, e) for p in pha for e in env], dtype=np.float32)
    kernels = hostlib.ctf_kernel_list(a.pixels, W.px, tr)
    orient = rng.integers(0, a.orientations, a.particles)
    sx, sy = rng.integers(-10, 11, a.particles), rng.integers(-10, 11, a.particles)
    X = E.window_shifts()
    ix = {int(x): i for i, x in enumerate(X)}
    req = np.zeros(a.particles, dtype=eng.SCAN_REQUEST_DTYPE)
    req["particle"], req["orient"], req["shiftX"], req["shiftY"] = np.arange(a.particles), orient, sx, sy
    print("%d records at %d^2 x %d candidates, batches of %d records, A at %d x %d cells%s"
          % (a.particles, a.pixels, G, E.max_batch()[0], len(X), len(X), (", " + a.label) if a.label else ""))

    def timed(call):
        E.set_phase_timing(True)
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        ph = E.phase_records()
        E.set_phase_timing(False)
        return out, [1e3 * ph["seconds"][ph["phase"] == k].sum() for k in range(3)], 1e3 * wall

    def run_a():
        """every (record, candidate) through the window entry; returns logp [n, G] and params [n, G] at the records' cells"""
        logp = np.zeros((a.particles, G))
        par = np.zeros((a.particles, G), dtype=eng.PARAM5_DTYPE)
        cell = (np.array([ix[int(v)] for v in sx]), np.array([ix[int(v)] for v in sy]))
        for g0 in range(0, G, nC):
            g1 = min(G, g0 + nC)
            lo = g1 - nC  # the last slice overlaps the one before: the handle takes exactly nC sets
            E.upload_ctf(kernels[lo:g1], tr[lo:g1])
            sets = np.arange(g0, g1) - lo
            wreq = np.zeros(a.particles * len(sets), dtype=eng.WINDOW_REQUEST_DTYPE)
            wreq["particle"] = np.repeat(np.arange(a.particles), len(sets))
            wreq["orient"] = np.repeat(orient, len(sets))
            wreq["conv"] = np.tile(sets, a.particles)
            t, p5 = E.window_posterior(wreq, want_params=True)
            t = t.reshape(a.particles, len(sets), len(X), len(X))
            logp[:, g0:g1] = t[np.arange(a.particles), :, cell[0], cell[1]]
            par[:, g0:g1] = p5.reshape(a.particles, len(sets))
        return logp, par

    def run_b():
        return E.ctf_scan(req, kernels, tr, want_params=True)

    first_b = run_b()  # first calls: staging buffers, code load
    first_a = None
    if not a.skip_a:
        first_a = run_a()
        d = np.abs(first_a[0] - first_b[0])
        ok = np.isfinite(first_a[0]) & np.isfinite(first_b[0])
        print("A and B: parameters bit for bit the same: %s; log posteriors equal in %d of %d finite pairs, largest "
              "difference %.3g" % (first_a[1].tobytes() == first_b[1].tobytes(), int((first_a[0][ok] == first_b[0][ok]).sum()),
                                   int(ok.sum()), float(d[ok].max()) if ok.any() else 0.0))
    tot = {"A": [], "B": []}
    for r in range(a.repeats):
        for what, call in (("A", run_a), ("B", run_b)):
            if what == "A" and a.skip_a:
                continue
            out, s, wall = timed(call)
            tot[what].append(sum(s))
            assert out[0].tobytes() == (first_a if what == "A" else first_b)[0].tobytes()
            names = ("projection", "conv and sums", "window pass") if what == "A" else ("projection", "preparation", "scan")
            print("run %d %s%s: device %.2f ms = %s %.2f + %s %.2f + %s %.2f ms; call(s) %.1f ms wall; %.3f us per (record, "
                  "candidate) on the device" % (r, what, (" " + a.label) if what == "B" and a.label else "", sum(s), names[0],
                                                s[0], names[1], s[1], names[2], s[2], wall, 1e3 * sum(s) / (a.particles * G)))
    for what in ("A", "B"):
        if tot[what]:
            v = np.array(tot[what])
            print("%s%s: device time median %.2f ms, min %.2f, max %.2f over %d runs"
                  % (what, (" " + a.label) if what == "B" and a.label else "", np.median(v), v.min(), v.max(), len(v)))
    if tot["A"]:
        print("A / B (medians): %.1f" % (np.median(tot["A"]) / np.median(tot["B"])))
    E.close()


if __name__ == "__main__":
    main()
