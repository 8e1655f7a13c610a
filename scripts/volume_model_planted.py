#!/usr/bin/env python3
"""The figures of the planted-object loop (reconstruct -> from_reconstruction -> upload_model_spectrum -> run) as
tests/test_volume_model_gpu.py::test_reconstruction_as_the_model_of_the_next_run prints them, recorded without a claim.
Runs that test on the device (or, with --from-log FILE, reads a pytest -s log of it) -> profiles/volume_model_planted.txt"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST = "tests/test_volume_model_gpu.py::test_reconstruction_as_the_model_of_the_next_run"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--from-log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_model_planted.txt"))
    a = ap.parse_args()
    if a.from_log:
        text = open(a.from_log).read()
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", TEST, "-q", "-s", "-p", "no:cacheprovider"], cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        text = r.stdout
        if r.returncode:
            sys.exit(text[-2000:])
    lines = [ln.lstrip(".") for ln in text.splitlines() if ln.lstrip(".").startswith("planted N=")]
    if not lines:
        sys.exit("the test printed no figures")
    with open(a.out, "w") as f:
        f.write("%s, one MI355X (scripts/volume_model_planted.py; recorded, no claim):\n" % TEST)
        f.write("40 spheres of radius 1.6 px, one noise-free particle per view over all CTF sets of the scene; Engine.reconstruct(want_spec=True)\n"
                "-> volume_model.from_reconstruction -> Engine.upload_model_spectrum(pad = 1), the same particles compared over the same\n"
                "orientations; exempt: particles whose two best log P in the CPU chain lie within the parity tolerance (cap 1 in 20)\n")
        f.write(lines[-1] + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
