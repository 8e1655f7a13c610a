"""The strip-lane column pass of the lean k_compare_fast of 16 k points (compare_fast.hpp, STRIP): during the column pass
a lane is (row of the block, column of a 16-column strip), wave w of a block takes columns 64 b + 16 w + c of ALL rows of
the block in round b, the conv operand comes through one descriptor over the block's rows, and the particle operand is
requested once per group of four row pairs and handed to the four lane rows through the head of the wave's own T region.
Nothing a (row, column) computes changes, so lean and full on one handle give the same probability block and angle table,
byte for byte (the harness of test_fast_lean.py); every case first makes sure that the second run really took the lean
kernel.  The lean kernels of other lengths keep lane = column and run the same cases: the strip kernel itself (16 k
points, H = 8 N1 + 1) meets 32^2, 48^2, 96^2, 224^2 and 240^2 here -- one column over a strip, waves without a column, a
9-column strip, one and two rounds -- and 80^2 ... 256^2 in test_fast_lean.py.

Shapes, all +-10 px, grid 1, chosen for where the mapping can go wrong (H = N / 2 + 1 columns):

    28^2, 30^2, 32^2   H = 15, 16, 17: a strip one short of full, the last strip exactly full, one column in wave 1
    24^2               13 columns: waves 1 .. 3 have no column at all
    48^2               25 columns: a 9-column strip in wave 1, waves 2 and 3 with none
    62^2, 94^2, 96^2   H = 32, 48, 49: whole strips only, and one column left for wave 3
    126^2              H = 64: exactly one full round
    224^2, 240^2       two rounds, the last 16 + 16 + 16 + 1 and 16 + 16 + 16 + 9 columns, N1 = 14 and odd N1 = 15
    200^2              the 8-point kernel (lane = column), two rounds, odd N1 = 25

(24 ... 62: a last block of at most 32 columns is split between the half-waves unless BIOEM_NO_SPLIT_LAST is set, and a
split launch is not a lean one.)  9 particles run the group-per-XCD block map, 65 the chunk map with a ragged chunk
(64 + 1); 3 x 3 = 9 rows leave one valid row in the last group of four, 5, 6 and 7 rows leave 1, 2 and 3.
"""
import functools

import numpy as np
import pytest

from test_fast_lean import N_ORIENT, full_then_lean, handle, run_all, run_own, stack

pytestmark = pytest.mark.gpu

SIG = {24: "k_compare_fast<10, 8, false, 1>", 48: "k_compare_fast<10, 16, false, 1>", 28: "k_compare_fast<10, 4, false, 1>",
       30: "k_compare_fast<10, 10, false, 1>", 32: "k_compare_fast<10, 16, false, 1>",
       62: "k_compare_fast<10, 2, false, 1>", 94: "k_compare_fast<10, 2, false, 1>",
       96: "k_compare_fast<10, 16, false, 1>", 126: "k_compare_fast<10, 18, false, 1>",
       200: "k_compare_fast<10, 8, false, 1>", 224: "k_compare_fast<10, 16, false, 1>",
       240: "k_compare_fast<10, 16, false, 1>"}
SIZES = [28, 30, 32, 24, 48, 62, 94, 96, 126, 224, 240, 200]


def unsplit(N, monkeypatch):
    """a last column block of at most 32 columns runs unsplit, i.e. lean, only with BIOEM_NO_SPLIT_LAST (read per launch)"""
    monkeypatch.delenv("BIOEM_NO_SPLIT_LAST", raising=False)
    H = N // 2 + 1
    if H - (H + 63) // 64 * 64 + 64 <= 32:
        monkeypatch.setenv("BIOEM_NO_SPLIT_LAST", "1")


def assert_same_blocks(full, lean, nP):
    nm = nP * 40
    assert full[:nm].tobytes() == lean[:nm].tobytes()  # probability entries
    assert full[nm:].tobytes() == lean[nm:].tobytes()  # angle table (WRITE_PROB_ANGLES)


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("nP", [9, 65])
@pytest.mark.parametrize("N", SIZES)
def test_lean_equals_full_at_every_strip_shape(N, nP, algo, monkeypatch):
    import bioem_amd.engine as eng
    unsplit(N, monkeypatch)
    W = stack(N)
    E = handle(W, nP, algo, write_angles=N_ORIENT)
    try:
        assert E.kernel_signature == SIG[N]
        full, lean = full_then_lean(E, run_all, True)  # (asserts that the second run launches the lean kernel)
        assert_same_blocks(full, lean, nP)
        pm = lean[:nP * 40].view(eng.PROB_MAP_DTYPE)
        assert np.all(np.isfinite(pm["Total"])) and np.all(pm["Total"] > 0)
    finally:
        E.close()


# ---- last groups of 1, 2 and 3 valid rows ----
@functools.lru_cache(maxsize=None)
def rows_stack(N, nOrient, nEnv):
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=9, nOrient=nOrient, nEnv=nEnv, maxD=10, npts=150)
    W.engine.close()
    assert W.nCTF == nEnv
    return W


def rows_handle(W, nOrient, algo):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import make_param_device
    pd = make_param_device(W.N, 10, 1, nOrient, W.steps, 1, W.px)
    pd.writeAngles = nOrient
    E = eng.Engine(pd, 9, nOrient, W.nCTF, algo=algo, device=0)
    E.upload_ctf(W.refCTF, W.ctfParam)
    E.upload_model(W.points, W.NormDen, W.px)
    E.upload_orientations(W.angles, True)
    E.upload_particle_maps(W.maps[:9])
    return E


def run_rows(nOrient):
    def run(E):
        import bioem_amd.engine as eng
        raw = eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)[0]
        E.start_run(raw)
        E.project_convolve_compare(0, nOrient)
        E.finish_run(raw)
        return raw
    return run


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("nOrient,nEnv", [(5, 1), (2, 3), (7, 1)], ids=["rows5", "rows6", "rows7"])
@pytest.mark.parametrize("N", [30, 96, 224])
def test_ragged_last_group(N, nOrient, nEnv, algo, monkeypatch):
    unsplit(N, monkeypatch)
    W = rows_stack(N, nOrient, nEnv)
    E = rows_handle(W, nOrient, algo)
    try:
        assert E.kernel_signature == SIG[N]
        full, lean = full_then_lean(E, run_rows(nOrient), True)
        assert_same_blocks(full, lean, 9)
    finally:
        E.close()


# ---- the own-list pass, one launch per batch and one per particle ----
@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N", [30, 96, 200, 224])
def test_own_list_pass_in_both_launch_modes(N, algo, monkeypatch):
    unsplit(N, monkeypatch)
    W = stack(N)
    E = handle(W, 9, algo, write_angles=N_ORIENT)
    try:
        assert E.kernel_signature == SIG[N]
        rng = np.random.default_rng(17)
        lists = []
        for p, n in enumerate([3, 1, 2, 3, 0, 3, 2, 1, 3]):  # ragged, one empty: blocks of 1, 2 and 3 valid rows
            q = W.angles[(np.arange(n) + p) % N_ORIENT] + rng.normal(size=(n, 4)).astype(np.float32) * 0.02
            lists.append((q / np.linalg.norm(q, axis=1)[:, None]).astype(np.float32))
        blocks = []
        for mode in ("batch", "particle"):
            E.set_own_launch(mode)
            E.upload_particle_orientation_lists(lists)
            if mode == "batch":
                assert E.own_kernel_signature == SIG[N].replace("k_compare_fast<", "k_compare_fast_own<")
            blocks += list(full_then_lean(E, run_own, True))
        assert all(b.tobytes() == blocks[0].tobytes() for b in blocks)
    finally:
        E.close()
