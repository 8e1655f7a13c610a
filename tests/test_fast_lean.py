"""The lean variant of k_compare_fast (compare_fast.hpp, template parameter LEAN): the instantiation of ONE path through
the kernel -- the whole static 21-row window, no split last column block -- which the host takes exactly where the full
instantiation's run-time tests would take that path (lean_launch_ok, bioem_hip.hip).  What a wave computes is the same
arithmetic in the same order, so on one handle and the same inputs

    Engine.set_compare_variant(False)  (full instantiations only)   and   (True)  (lean where a launch qualifies)

must give the same probability block and, with WRITE_PROB_ANGLES, the same angle table, byte for byte; the setter's
return value says whether the second run really took a lean kernel, so that the comparison is not full against full.

Orientation lists are 3 orientations x 3 CTFs = 9 rows (the last group of four is ragged); 9 particles run the
group-per-XCD block map with its padding blocks, 72 the chunk map (64 + 8).  Shapes, all +-10 px, grid 1:

    80^2    one column block of 41 columns, N1 = 5       224^2  the headline instantiation's own shape
    112^2   one block, N1 = 7                            128^2  <10, 16, true, 1>: the Nyquist tail in lean form
    208^2   two blocks, the last of 41 columns, N1 = 13  256^2  the same with two blocks

and where the kernel's own tests take another path the setter must say 0 and nothing may change: 144^2 and 160^2 (split
last block), 224^2 +-9 px (19 displacements on the 21-row kernel).  BIOEM_NO_SPLIT_LAST is read per launch: with it 160^2
runs unsplit and lean.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ORIENT, N_ENV = 3, 3
FULL_21 = "k_compare_fast<10, 16, false, 1>"
NYQ_21 = "k_compare_fast<10, 16, true, 1>"
LEAN_SHAPES = [(80, FULL_21), (112, FULL_21), (208, FULL_21), (224, FULL_21), (128, NYQ_21), (256, NYQ_21)]


@functools.lru_cache(maxsize=None)
def stack(N):
    """the data of a shape, made once: model, CTFs, orientations and 72 rendered particles (the 9-particle handles take
    the first nine); the workload's own handle is closed, every test opens the handles it needs"""
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=72, nOrient=N_ORIENT, nEnv=N_ENV, maxD=10, npts=150)
    W.engine.close()
    assert W.nCTF == 3
    return W


def handle(W, nP, algo, maxD=10, write_angles=0):
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import make_param_device
    pd = make_param_device(W.N, maxD, 1, N_ORIENT, W.steps, 1, W.px)
    pd.writeAngles = int(write_angles)
    E = eng.Engine(pd, nP, N_ORIENT, W.nCTF, algo=algo, device=0)
    E.upload_ctf(W.refCTF, W.ctfParam)
    E.upload_model(W.points, W.NormDen, W.px)
    E.upload_orientations(W.angles, True)
    E.upload_particle_maps(W.maps[:nP])
    return E


def run_all(E):
    import bioem_amd.engine as eng
    raw = eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)[0]
    E.start_run(raw)
    E.project_convolve_compare(0, N_ORIENT)
    E.finish_run(raw)
    return raw


def run_own(E):
    import bioem_amd.engine as eng
    raw = eng.new_prob_block(E.nMaps, E.nAngles, E.pd.writeAngles)[0]
    E.start_run(raw)
    E.compare_own_orientations(0, E.nMaps)
    E.finish_run(raw)
    return raw


def full_then_lean(E, run, expect_lean):
    """the same pass under both variants of one handle: (full, lean) blocks, the setter's answers and labels checked"""
    sig = E.kernel_signature
    assert E.set_compare_variant(False) is False  # no launch of the handle takes a lean kernel now
    full = run(E).copy()
    assert E.set_compare_variant(True) is expect_lean
    lean = run(E).copy()
    assert E.kernel_signature == sig  # the label names the instantiation's template arguments, not the variant
    return full, lean


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("nP", [9, 72])
@pytest.mark.parametrize("N,sig", LEAN_SHAPES, ids=["n%d" % s[0] for s in LEAN_SHAPES])
def test_lean_launch_equals_full_bit_for_bit(N, sig, nP, algo):
    import bioem_amd.engine as eng
    W = stack(N)
    E = handle(W, nP, algo, write_angles=N_ORIENT)
    try:
        assert E.kernel_signature == sig
        assert E.set_compare_variant(True) is True  # the default of the handle, said once more
        full, lean = full_then_lean(E, run_all, True)
        nm = nP * 40
        assert full[:nm].tobytes() == lean[:nm].tobytes()   # probability entries
        assert full[nm:].tobytes() == lean[nm:].tobytes()   # angle table (WRITE_PROB_ANGLES)
        pm = lean[:nm].view(eng.PROB_MAP_DTYPE)
        assert np.all(np.isfinite(pm["Total"])) and np.all(pm["Total"] > 0)
    finally:
        E.close()


NOT_LEAN = [(144, 10, "split_last_block"), (160, 10, "split_last_block_17_columns"), (224, 9, "19_displacements")]


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N,maxD,what", NOT_LEAN, ids=[s[2] for s in NOT_LEAN])
def test_launches_that_take_another_path_stay_full(N, maxD, what, algo, monkeypatch):
    monkeypatch.delenv("BIOEM_NO_SPLIT_LAST", raising=False)
    W = stack(N)
    E = handle(W, 9, algo, maxD=maxD, write_angles=N_ORIENT)
    try:
        assert E.kernel_signature == FULL_21
        full, lean = full_then_lean(E, run_all, False)
        assert full.tobytes() == lean.tobytes()
        if N == 160:
            # the choice is made per launch, after the launch's `split` is known: unsplit, the same handle runs lean --
            # against its own unsplit full run
            monkeypatch.setenv("BIOEM_NO_SPLIT_LAST", "1")
            ufull, ulean = full_then_lean(E, run_all, True)
            assert ufull.tobytes() == ulean.tobytes()
            monkeypatch.delenv("BIOEM_NO_SPLIT_LAST")
            assert E.set_compare_variant(True) is False
            assert run_all(E).tobytes() == full.tobytes()
    finally:
        E.close()


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N", [112, 224])
def test_own_list_pass_batch_and_per_particle_under_both_variants(N, algo):
    """own-list pass: the batch launch (k_compare_fast on OwnCompareArgs, its lean row of kernels_fast_own.hip) and the
    per-particle launches of the plan's kernel, each under both variants: four equal blocks"""
    W = stack(N)
    E = handle(W, 9, algo, write_angles=N_ORIENT)
    try:
        rng = np.random.default_rng(11)
        lists = []
        for p, n in enumerate([3, 1, 2, 3, 0, 3, 2, 1, 3]):  # ragged, one empty
            q = W.angles[(np.arange(n) + p) % N_ORIENT] + rng.normal(size=(n, 4)).astype(np.float32) * 0.02
            lists.append((q / np.linalg.norm(q, axis=1)[:, None]).astype(np.float32))
        blocks = {}
        for mode in ("batch", "particle"):
            E.set_own_launch(mode)
            E.upload_particle_orientation_lists(lists)
            if mode == "batch":
                assert E.own_kernel_signature == FULL_21.replace("k_compare_fast<", "k_compare_fast_own<")
            blocks[mode] = full_then_lean(E, run_own, True)
        ref = blocks["batch"][0].tobytes()
        assert all(b.tobytes() == ref for pair in blocks.values() for b in pair)
    finally:
        E.close()


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("N", [208, 224])
def test_lean_launch_against_oracle(N, algo):
    """the tolerance tests/test_sym_window.py applies to this kernel (assert_workload_matches), on the lean launch"""
    from test_gpu_parity import assert_workload_matches, oracle_on_workload
    import bioem_amd.engine as eng
    W = stack(N)
    sel = [0, 1, 2]
    E = handle(W, 3, algo)
    try:
        assert E.set_compare_variant(True) is True
        want, const = oracle_on_workload(W, sel, N_ORIENT, algo, engine=E, maps=W.maps[:3])
        got = run_all(E)[:3 * 40].view(eng.PROB_MAP_DTYPE)
        print(N, algo, [float(np.log(g["Total"]) + g["Constoadd"]) for g in got],
              [float(np.log(w["Total"]) + w["Constoadd"]) for w in want])
        assert_workload_matches(got, want, const, sel)
    finally:
        E.close()
