"""The static 21-row window pass of k_compare_fast over |dy| (window_accumulate_sym, compare_fast.hpp): every lane owns
one dx row and four |dy|, and forms cc[dx][+dy] = A - B and cc[dx][-dy] = A + B from sums over a tabulated cos | sin
matrix.  Against the CPU oracle, 3 particles x 3 orientations x 2 CTFs, ALGO 1 and 2, at the sizes where the pass takes
another path:

    32^2   one column block                      144^2  split last block
    96^2   H = 49: half-empty last column pair   192^2  Nyquist term + split last block
    128^2  Nyquist term                          224^2  table slice reloaded for a second, partly filled block
    64^2 +-20 px grid 2   row stride 2 (the |dy| of the table are multiples of the stride)
    42^2 +-16 px          2 x 2 tiles of 21 rows: the ndx / ndy masks of the tiles

log P is a log-sum-exp over the window and does not change when +dy and -dy are swapped, so a sign error in B would pass
a comparison of log P alone.  Each shape therefore also runs particles rendered from a projection moved by an
asymmetric displacement -- (+3, -7), (-10, +1) and the window's corner (+maxD, -maxD), in window rows -- at a
signal-to-noise ratio of 1, where the posterior peak is that displacement: the oracle must find it, untied (it does, for
every shape and both algorithms: (cent_x, cent_y) = the plant, orientation p, CTF p mod 2), and the engine must return the
oracle's (orient, conv, cent_x, cent_y) exactly.
"""
import math

import numpy as np
import pytest

from test_gpu_parity import assert_workload_matches, oracle_on_workload, run_workload

pytestmark = pytest.mark.gpu

# (N, maxD, grid, kernel the plan must select: a 21-row instantiation that takes the pass, compare_args.hpp)
SHAPES = [
    (32, 10, 1, "k_compare_fast<10, 16, false, 1>"),
    (96, 10, 1, "k_compare_fast<10, 16, false, 1>"),
    (128, 10, 1, "k_compare_fast<10, 16, true, 1>"),
    (144, 10, 1, "k_compare_fast<10, 16, false, 1>"),
    (192, 10, 1, "k_compare_fast<10, 16, true, 1>"),
    (224, 10, 1, "k_compare_fast<10, 16, false, 1>"),
    (64, 20, 2, "k_compare_fast<10, 16, true, 2>"),
    (42, 16, 1, "k_compare_fast<10, 6, false, 1> x 2^2 tiles of 21 rows"),
]
PLANTS = [(3, -7), (-10, 1)]  # window rows (times the grid spacing = pixels); the third plant is the window's corner


def planted_particles(W, shifts, snr=1.0, seed=20261018):
    """particle p = projection of orientation p under CTF p mod nCTF, moved by shifts[p] pixels, plus unit noise"""
    N = W.N
    maps = np.zeros((len(shifts), N, N), dtype=np.float32)
    for p, (sx, sy) in enumerate(shifts):
        spec, _, _ = W.engine.debug_convolution(p % W.nOrient, p % W.nCTF)
        img = np.fft.irfft2(spec[..., 0] + 1j * spec[..., 1], s=(N, N))
        img = (img - img.mean()) / img.std()
        img = np.roll(img, (sx, sy), axis=(0, 1)) * math.sqrt(snr) + np.random.default_rng(seed + p).normal(size=(N, N))
        maps[p] = ((img - img.mean()) / img.std()).astype(np.float32)
    return maps


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_d%d_g%d" % s[:3])
def test_window_pass_over_abs_dy_against_oracle(shape, algo):
    from bioem_amd.synthetic import Workload
    import ctypes as C
    N, d, g, sig = shape
    W = Workload(N=N, nP=3, nOrient=3, nEnv=2, maxD=d, grid=g, algo=algo, npts=150)
    try:
        buf = C.create_string_buffer(512)
        assert W.engine.L.bioem_hip_plan(N, d, g, algo, buf, 512) == 0 and buf.value.decode() == sig
        assert W.engine.kernel_signature == sig.split(" x ")[0]
        sel = [0, 1, 2]
        # the stack of the synthetic workload: random shifts, signal-to-noise ratio 0.05
        want, const = oracle_on_workload(W, sel, 3, algo)
        _, got = run_workload(W, 0, 3)
        print("noisy  ", shape[:3], algo, [(int(w["orient"]), int(w["conv"]), int(w["cent_x"]), int(w["cent_y"]),
                                            float(np.log(w["Total"]) + w["Constoadd"])) for w in want],
              [(int(w["orient"]), int(w["conv"]), int(w["cent_x"]), int(w["cent_y"]),
                float(np.log(w["Total"]) + w["Constoadd"])) for w in got])
        assert_workload_matches(got, want, const, sel)
        # planted peaks
        shifts = [(sx * g, sy * g) for sx, sy in PLANTS + [(d // g, -(d // g))]]
        maps = planted_particles(W, shifts)
        W.engine.upload_particle_maps(maps)
        want, const = oracle_on_workload(W, sel, 3, algo, maps=maps)
        _, got = run_workload(W, 0, 3)
        print("planted", shape[:3], algo, shifts, [(int(w["orient"]), int(w["conv"]), int(w["cent_x"]), int(w["cent_y"]))
                                                   for w in want],
              [(int(w["orient"]), int(w["conv"]), int(w["cent_x"]), int(w["cent_y"])) for w in got])
        for p, (sx, sy) in enumerate(shifts):
            assert (int(want[p]["orient"]), int(want[p]["conv"])) == (p, p % W.nCTF)
            assert (int(want[p]["cent_x"]), int(want[p]["cent_y"])) == (sx, sy)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()
