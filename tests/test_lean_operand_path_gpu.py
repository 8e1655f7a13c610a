"""The operand path of the lean k_compare_fast (compare_fast.hpp) and the line-aligned row-pair pitch (bioem_hip.hip,
line_aligned_pitch), both of which move addresses and no value.

1. Lean against full on one handle (the harness of test_fast_lean.py: 3 orientations x 3 CTFs, 9 and 72 particles, +-10 px,
   ALGO 1 and 2, probability block and angle table as bytes) at the shapes where the lean loop's addressing can go wrong
   and that file does not run.  In the lean loop the lane offset is constant over a column block and the last RD requests
   of a k1 step take their row from one scalar base chosen per step -- the next step, the next block 1 024 bytes on, or
   rows 0 .. RD - 1 of the block again after the last one:

       32^2   <10, 16>  N1 = 2: the tail requests wrap in the second step already (unsplit: BIOEM_NO_SPLIT_LAST)
       24^2   <10, 8>   R / 2 = RD = 4: every request of a step is one of its last RD; N1 = 3 (unsplit likewise)
       34^2   <10, 2>   a ring of one, N1 = 17 (unsplit likewise)
       96^2   <10, 16>  one block of 49 columns, masked lanes
       200^2  <10, 8>   two blocks, the last of 37 columns, odd N1 = 25
       240^2  <10, 16>  two blocks, 57 columns, odd N1 = 15

   No lean shape has a single k1 step (N = R <= 18 is smaller than the 21-row window): 32^2, two steps, is the shortest.
2. The default pitch against BIOEM_NO_PITCH_PAD=1 at the sizes the rule pads among 96^2, 200^2, 224^2 and 240^2: the
   probability block, the particle spectra and a convolution batch, byte for byte, and the pitch itself.
3. One analysis entry per kernel family on a handle of a newly padded size against the same call on an unpadded handle.
"""
import functools

import numpy as np
import pytest

import convolution_reference as cr
from test_fast_lean import N_ORIENT, full_then_lean, handle, run_all, run_own, stack

pytestmark = pytest.mark.gpu

SHAPES = [(32, "k_compare_fast<10, 16, false, 1>", True), (24, "k_compare_fast<10, 8, false, 1>", True),
          (34, "k_compare_fast<10, 2, false, 1>", True), (96, "k_compare_fast<10, 16, false, 1>", False),
          (200, "k_compare_fast<10, 8, false, 1>", False), (240, "k_compare_fast<10, 16, false, 1>", False)]


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("nP", [9, 72])
@pytest.mark.parametrize("N,sig,unsplit", SHAPES, ids=["n%d" % s[0] for s in SHAPES])
def test_lean_equals_full_where_the_ring_wraps(N, sig, unsplit, nP, algo, monkeypatch):
    monkeypatch.delenv("BIOEM_NO_SPLIT_LAST", raising=False)
    if unsplit:  # (a last block of at most 32 columns is split between the half-waves otherwise: not a lean launch)
        monkeypatch.setenv("BIOEM_NO_SPLIT_LAST", "1")
    W = stack(N)
    E = handle(W, nP, algo, write_angles=N_ORIENT)
    try:
        assert E.kernel_signature == sig
        full, lean = full_then_lean(E, run_all, True)
        nm = nP * 40
        assert full[:nm].tobytes() == lean[:nm].tobytes()
        assert full[nm:].tobytes() == lean[nm:].tobytes()
    finally:
        E.close()


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N", [96, 240])
def test_own_list_pass_in_both_launch_modes(N, algo):
    W = stack(N)
    E = handle(W, 9, algo, write_angles=N_ORIENT)
    try:
        rng = np.random.default_rng(5)
        lists = []
        for p, n in enumerate([3, 1, 2, 3, 0, 3, 2, 1, 3]):
            q = W.angles[(np.arange(n) + p) % N_ORIENT] + rng.normal(size=(n, 4)).astype(np.float32) * 0.02
            lists.append((q / np.linalg.norm(q, axis=1)[:, None]).astype(np.float32))
        blocks = []
        for mode in ("batch", "particle"):
            E.set_own_launch(mode)
            E.upload_particle_orientation_lists(lists)
            blocks += list(full_then_lean(E, run_own, True))
        assert all(b.tobytes() == blocks[0].tobytes() for b in blocks)
    finally:
        E.close()


# ---- the pitch rule, stated on its own ----
def rule_pitch(N):
    """row-pair pitch in 16-byte words of an untiled k_compare_fast / fastm / fastm2 plan"""
    H = N // 2 + 1
    if N % 64 == 0 and N >= 192:
        return H + 15
    if N < 160:  # (96^2 lost 0.6 % with it: the rule starts at the smallest size that gained)
        return H
    Hp = (H + ALIGN - 1) // ALIGN * ALIGN
    return Hp + ALIGN if Hp % 32 == 0 else Hp


ALIGN = 8
PADDED = [N for N in (96, 200, 224, 240) if rule_pitch(N) != N // 2 + 1]


def test_rule_pads_these_sizes():
    assert PADDED == [200, 224, 240] and rule_pitch(96) == 49 and rule_pitch(160) == 88
    for N in PADDED:
        Hp, H = rule_pitch(N), N // 2 + 1
        assert H < Hp <= H + 15 and (16 * Hp) % 128 == 0 and (16 * Hp) % 512 != 0


@functools.lru_cache(maxsize=None)
def both_layouts(N):
    """what a 9-particle handle of the default pitch and one at pitch H (BIOEM_NO_PITCH_PAD, read when the handle is
    created) hand out: probability block, particle spectra, one convolution batch, and the analysis entries"""
    import os
    import bioem_amd.engine as eng
    W = stack(N)
    out = []
    for plain in (False, True):
        old = os.environ.pop("BIOEM_NO_PITCH_PAD", None)
        if plain:
            os.environ["BIOEM_NO_PITCH_PAD"] = "1"
        try:
            E = handle(W, 9, 1, write_angles=N_ORIENT)
        finally:
            os.environ.pop("BIOEM_NO_PITCH_PAD", None)
            if old is not None:
                os.environ["BIOEM_NO_PITCH_PAD"] = old
        try:
            assert E.set_compare_variant(True) is True
            r = {"block": run_all(E).copy()}
            pmap = r["block"][:9 * 40].view(eng.PROB_MAP_DTYPE).copy()
            r["particles"] = E.debug_particles()
            spec = E.debug_projection_maps(0, 2, want_spec=True)[2]  # (a batch is at most max_batch - 1 rows and a guard)
            r["conv"], r["params"], r["raw"], r["info"] = E.debug_convolve_batch(spec, 0, W.nCTF, want_raw=True)
            r["maps"] = E.render_best_maps(pmap)
            r["rings"] = E.best_match_rings(pmap)
            r["window"] = E.best_match_window(pmap, want_cc=True)
            r["views"] = E.view_sums(pmap, np.arange(9, dtype=np.int32) % 3)
            r["scan"] = E.best_match_ctf_scan(pmap, W.refCTF, W.ctfParam, want_cc=True)
            out.append(r)
        finally:
            E.close()
    return out


def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", PADDED)
def test_default_pitch_equals_pitch_H_bit_for_bit(N, monkeypatch):
    monkeypatch.delenv("BIOEM_NO_PITCH_PAD", raising=False)
    pad, plain = both_layouts(N)
    H = N // 2 + 1
    assert pad["info"]["Hp"] == rule_pitch(N) and plain["info"]["Hp"] == H, (pad["info"], plain["info"])
    assert same(pad["block"], plain["block"])
    assert same(pad["particles"], plain["particles"])
    assert same(pad["conv"], plain["conv"]) and same(pad["params"], plain["params"])
    rows = pad["info"]["rows"]
    for r in range(rows):
        for side in (pad, plain):
            i = side["info"]
            assert side["raw"].shape == (rows, N * i["Hp"], 2)
            # the bins of the raw row, and only those, are the data: columns [H, Hp) of a row pair hold none
            want, at = cr.comparison_layout(side["conv"][r], i["fast"], i["N1"], i["Hp"])
            assert int(at.sum()) == N * H
            assert side["raw"][r][at].tobytes() == want[at].tobytes()
            back = cr.from_comparison_layout(side["raw"][r], N, i["fast"], i["N1"], i["Hp"])
            assert back.tobytes() == plain["conv"][r].tobytes()


@pytest.mark.parametrize("entry", ["maps", "rings", "window", "views", "scan"])
def test_analysis_entries_on_a_padded_handle(entry, monkeypatch):
    monkeypatch.delenv("BIOEM_NO_PITCH_PAD", raising=False)
    pad, plain = both_layouts(224)
    assert pad["info"]["Hp"] > 113 and plain["info"]["Hp"] == 113
    assert same(pad[entry], plain[entry]), entry
