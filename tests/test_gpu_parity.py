"""GPU parity tests (run on the MI355X box): the HIP engine, called through the C ABI, against the CPU oracle
on the same inputs, against the committed reference outputs (tests/golden/), and -- at the benchmark's full
size -- through size-independent properties.

Tolerance (north_star): |log P_gpu - log P_oracle| <= 1e-4 * |log P| and an identical maximising tuple.
Observed differences are float rounding of the transforms: <= 3e-3 absolute at 224^2 (4e-8 relative), so a
tighter absolute bound of 2e-2 is asserted as well.
"""
import os
import subprocess

import numpy as np
import pytest

import io_formats as iof
import oracle as orc
from golden_util import CASES, golden_output, load_case, oracle_setup, write_case_inputs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4
ABS_TOL = 2e-2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pd_of(S):
    import bioem_amd.engine as eng
    pd = eng.ParamDevice()
    for f, _ in eng.ParamDevice._fields_:
        setattr(pd, f, getattr(S.pd, f))
    return pd


def make_engine(S, algo, real_space_particles=False):
    import bioem_amd.engine as eng
    E = eng.Engine(pd_of(S), S.nMaps, S.nAngles, S.nCTF, algo=algo, device=0)
    if real_space_particles:
        E.upload_particle_maps(S.maps)
    else:
        E.upload_particles(S.refFFT, S.sumRef, S.sumsqRef)
    E.upload_ctf(S.refCTF, S.ctfParam)
    E.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
    E.upload_orientations(S.angles, S.isQuat)
    return E


def run_native(E, S, o0=0, o1=None):
    import bioem_amd.engine as eng
    raw, pmap, pang = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
    E.start_run(raw)
    E.project_convolve_compare(o0, S.nAngles if o1 is None else o1)
    E.finish_run(raw)
    return raw, pmap, pang


def assert_same_posterior(S, got, want):
    for a, b in zip(got, want):
        la, lb = S.final_logp(a), S.final_logp(b)
        assert abs(la - lb) <= REL_TOL * abs(lb), (la, lb)
        assert abs(la - lb) <= ABS_TOL, (la, lb)
        assert (a["orient"], a["conv"], a["cent_x"], a["cent_y"]) == (b["orient"], b["conv"], b["cent_x"], b["cent_y"])
        assert abs(a["norm"] - b["norm"]) <= 1e-4 * max(1.0, abs(b["norm"]))
        assert abs(a["mu"] - b["mu"]) <= 1e-4 * max(1.0, abs(b["mu"]))


_cache = {}


def setup_for(name):
    if name not in _cache:
        case = load_case(name)
        _cache[name] = (case, oracle_setup(case))
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_native_path_matches_oracle_and_reference(name):
    """project -> convolve -> compare entirely on the device, every golden case, ALGO 1 and 2."""
    case, S = setup_for(name)
    for algo in case["algos"]:
        E = make_engine(S, algo)
        assert E.fast_path == (S.N % 2 == 0)
        _, pmap, _ = run_native(E, S)
        want, _ = S.run(algo)
        assert_same_posterior(S, pmap, want)
        # and against the reference's own Output_Probabilities
        gold = iof.parse_output_probabilities(golden_output(case, algo))
        mine = iof.parse_output_probabilities(orc.format_output_probabilities(S, pmap))
        for g, m in zip(gold, mine):
            assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
            assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])
        E.close()


@pytest.mark.parametrize("name", ["g10_n64", "g1_n48", "g7_n224", "g20_n256"])  # (256^2: the padded pitch)
def test_reference_compatible_compare_entry(name):
    """bioem_hip_compare == bioem::compareRefMaps: host-prepared conv spectra in the 2-slot pipeline buffers
    (bioem.cpp:825-853), several convs per call, asynchronous enqueue."""
    import bioem_amd.engine as eng
    case, S = setup_for(name)
    E = make_engine(S, 1)
    nPar = min(3, S.nCTF)                       # nTotParallelConv
    conv_base = np.zeros((2 * nPar, S.N, S.H, 2), dtype=np.float32)
    par_base = np.zeros(2 * nPar, dtype=eng.PARAM5_DTYPE)
    raw, pmap, _ = eng.new_prob_block(S.nMaps, S.nAngles, 0)
    E.start_run(raw)
    want = S.new_prob()[0]
    nO = min(S.nAngles, 6)
    ipipe = 0
    for io in range(nO):
        conv, p5 = S.conv_spectra(io)
        for c0 in range(0, S.nCTF, nPar):
            n = min(nPar, S.nCTF - c0)
            k = (ipipe & 1) * nPar
            conv_base[k:k + n] = conv[c0:c0 + n]
            par_base[k:k + n] = p5[c0:c0 + n]
            E.compare(ipipe, io, c0, n, nPar, conv_base, par_base)
            S.compare(1, io, c0, conv[c0:c0 + n], p5[c0:c0 + n], want)
            ipipe += 1
    E.finish_run(raw)
    assert_same_posterior(S, pmap, want)
    E.close()


@pytest.mark.parametrize("name,split_ctf", [("g10_n64", False), ("g4_n32_angles", True), ("g2_n128", False),
                                            ("g13_n32_psf_writectf", True), ("g20_n256", True)])
def test_staged_device_entries_equal_the_fused_entry(name, split_ctf):
    """bioem_hip_project / _convolve / _compare_device (createProjection, createConvolutedProjectionMap and compareRefMaps
    as separate asynchronous batched entries, everything device-resident) against bioem_hip_project_convolve_compare
    over the same (orientation, CTF) rows in the same order: bit-identical probability blocks (also the angle table), and
    the oracle agrees.  Batches of three orientations alternate between the two buffer sets; with split_ctf every batch
    is convolved and compared in two CTF ranges."""
    import bioem_amd.engine as eng
    case, S = setup_for(name)
    algo = case["algos"][0]
    E = make_engine(S, algo)
    batches = [(o, min(o + 3, S.nAngles)) for o in range(0, S.nAngles, 3)]
    cut = max(1, S.nCTF // 2)
    ranges = [(0, cut), (cut, S.nCTF)] if (split_ctf and S.nCTF > 1) else [(0, S.nCTF)]
    raw_f, pmap_f, _ = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
    E.start_run(raw_f)
    for o0, o1 in batches:
        for c0, c1 in ranges:
            E.project_convolve_compare_ctf(o0, o1, c0, c1)
    E.finish_run(raw_f)
    raw_s, pmap_s, _ = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
    E.start_run(raw_s)
    for b, (o0, o1) in enumerate(batches):
        E.project(b, o0, o1)
        for c0, c1 in ranges:
            E.convolve(b, c0, c1)
            E.compare_device(b)
    E.finish_run(raw_s)
    assert raw_s.tobytes() == raw_f.tobytes()
    want, _ = S.run(algo)
    assert_same_posterior(S, pmap_s, want)
    maxO, maxRows = E.max_batch()
    assert maxO >= 1 and maxRows >= S.nCTF
    # error behaviour: stages out of order or beyond the capacity of a buffer set are refused with a message
    E2 = make_engine(S, algo)
    with pytest.raises(RuntimeError, match="bioem_hip_project first"):
        E2.convolve(0, 0, S.nCTF)
    with pytest.raises(RuntimeError, match="bioem_hip_project and bioem_hip_convolve first"):
        E2.compare_device(1)
    with pytest.raises(RuntimeError, match="range invalid"):
        E2.project(0, 0, S.nAngles + 1)
    # the fused entry overwrites both buffer sets: what was staged before it is gone
    raw_2, _, _ = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
    E2.start_run(raw_2)
    E2.project(0, 0, min(3, S.nAngles))
    E2.convolve(0, 0, S.nCTF)
    E2.project_convolve_compare(0, S.nAngles)
    with pytest.raises(RuntimeError, match="bioem_hip_project and bioem_hip_convolve first"):
        E2.compare_device(0)
    E2.close()
    E.close()


@pytest.mark.parametrize("name,ring,order", [("g4_n32_angles", 4, "orient"), ("g4_n32_angles", 3, "ctf"),
                                             ("g10_n64", 5, "orient"), ("g8_n32_grid", 1, "orient"),
                                             ("g11_n32_eulerlist", 7, "ctf")])
def test_compare_entry_ring_ragged_flushes(name, ring, order, monkeypatch):
    """The reference-compatible entry stages rows into a ring and launches one comparison per filled half.  Small
    rings (BIOEM_COMPAT_RING rows per half) make launches start in the middle of a call and in the middle of an
    orientation's CTFs; order "ctf" walks the CTF blocks in the outer loop, so every orientation returns after other
    ones were staged (the WRITE_PROB_ANGLES runs must then not be split inside one launch).  Folding in call order,
    the particle entries AND the angle table must match the oracle fed with the same call sequence; one conv per
    call = the reference's default ALGO-1 loop (nTotParallelConv = 1, bioem.cpp:534)."""
    import bioem_amd.engine as eng
    monkeypatch.setenv("BIOEM_COMPAT_RING", str(ring))
    case, S = setup_for(name)
    for algo in case["algos"]:
        E = make_engine(S, algo)
        nPar = 1 if ring == 1 else min(3, S.nCTF)
        conv_base = np.zeros((2 * nPar, S.N, S.H, 2), dtype=np.float32)
        par_base = np.zeros(2 * nPar, dtype=eng.PARAM5_DTYPE)
        raw, pmap, pang = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
        E.start_run(raw)
        want, wang = S.new_prob()
        calls = [(io, c0) for io in range(S.nAngles) for c0 in range(0, S.nCTF, nPar)]
        if order == "ctf":
            calls = [(io, c0) for c0 in range(0, S.nCTF, nPar) for io in range(S.nAngles)]
        convs = {}
        for ipipe, (io, c0) in enumerate(calls):
            if io not in convs:
                convs[io] = S.conv_spectra(io)
            conv, p5 = convs[io]
            n = min(nPar, S.nCTF - c0)
            k = (ipipe & 1) * nPar
            conv_base[k:k + n] = conv[c0:c0 + n]
            par_base[k:k + n] = p5[c0:c0 + n]
            E.compare(ipipe, io, c0, n, nPar, conv_base, par_base)
            conv_base[k:k + n] = 7.0        # the slot is the caller's again as soon as the call returns
            S.compare(algo, io, c0, conv[c0:c0 + n], p5[c0:c0 + n], want, wang)
        E.finish_run(raw)
        assert_same_posterior(S, pmap, want)
        if S.pd.writeAngles:
            la = np.log(pang["forAngles"]) + pang["ConstAngle"]
            lb = np.log(wang["forAngles"]) + wang["ConstAngle"]
            assert np.abs(la - lb).max() <= 5e-3
        E.close()


@pytest.mark.parametrize("name", ["g10_n64", "g9_n35_odd", "g6_n32_euler", "g7_n224"])
def test_device_projection_and_convolution(name):
    """createProjection / createConvolutedProjectionMap on the device vs the oracle (spectra, sumC, sumsquareC)."""
    case, S = setup_for(name)
    E = make_engine(S, 1)
    for io in [0, S.nAngles // 2, S.nAngles - 1]:
        spec = E.debug_projection(io)
        ref = orc.projection(S.points, S.NormDen, S.angles[io], S.isQuat, S.N, S.px, S.P["shiftX"], S.P["shiftY"])
        scale = np.abs(ref).max()
        assert np.abs(spec - ref).max() <= 2e-6 * scale
        conv, p5 = S.conv_spectra(io)
        for c in [0, S.nCTF - 1]:
            got, sC, ssC = E.debug_convolution(io, c)
            assert np.abs(got - conv[c]).max() <= 2e-6 * np.abs(conv[c]).max()
            assert abs(sC - p5[c]["sumC"]) <= 2e-6 * abs(p5[c]["sumC"])
            assert abs(ssC - p5[c]["sumsquareC"]) <= 1e-5 * abs(p5[c]["sumsquareC"])
    E.close()


R2C_SIZES = [16, 20, 35, 44, 48, 50, 64, 75, 96, 100, 120, 128, 133, 144, 160, 180, 192, 200, 224, 225, 240, 256, 280, 288,
             300, 304, 320, 360, 380, 400]


@pytest.mark.parametrize("N", R2C_SIZES)
def test_fast_r2c_against_numpy_and_the_exact_dft(N, monkeypatch):
    """The r2c of projections and particle maps (r2c_fft.hpp: one split N = A * B, register FFTs of A and B points in
    double) against numpy's double transform rounded to float -- what fftwf_plan_dft_r2c_2d (bioem.cpp:1848,
    map.cpp:585) approximates -- and against the exact-DFT kernels of rounds 1-3 (BIOEM_R2C=dft): the same rounded
    values but for a few last-bit flips.  Sizes: every sub-transform length 2...20 as A and as B, odd N, the BASELINE
    sizes; 7 images so that a block's group of rows / columns runs over image boundaries and ends ragged."""
    from bioem_amd import engine as eng
    rng = np.random.default_rng(N)
    img = rng.standard_normal((7, N, N)).astype(np.float32) + np.float32(0.3)
    want = np.fft.rfft2(img.astype(np.float64))
    monkeypatch.delenv("BIOEM_R2C", raising=False)
    fast = eng.r2c(img)
    scale = np.abs(want).max()
    assert np.abs(fast - want).max() <= 1.5e-7 * scale          # float rounding of the exact result: 6e-8 of a value
    monkeypatch.setenv("BIOEM_R2C", "dft")
    slow = eng.r2c(img)
    assert np.abs(slow - want).max() <= 1.5e-7 * scale
    # bins that are zero in exact arithmetic (imaginary parts of the self-conjugate ones) are rounding noise in both
    differ = np.count_nonzero(fast.view(np.float32) != slow.view(np.float32))
    assert differ <= 0.02 * fast.size * 2, differ


@pytest.mark.parametrize("name", ["g10_n64", "g9_n35_odd", "g7_n224", "g19_n200"])
def test_fused_convolution_equals_the_two_kernel_one(name, monkeypatch):
    """k_convolve_sums (few particles) and k_convolve + k_parseval_ordered (many) are the same arithmetic in the same
    order: spectra, sumC and sumsquareC agree to the bit for every CTF."""
    case, S = setup_for(name)
    E = make_engine(S, 1)
    for io in [0, S.nAngles - 1]:
        for c in range(S.nCTF):
            monkeypatch.setenv("BIOEM_CONVOLVE_FUSED", "1")
            a = E.debug_convolution(io, c)
            monkeypatch.setenv("BIOEM_CONVOLVE_FUSED", "0")
            b = E.debug_convolution(io, c)
            assert a[0].tobytes() == b[0].tobytes()
            assert np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes()
            assert np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes()
    E.close()


@pytest.mark.parametrize("name", ["g2_n128", "g7_n224", "g19_n200", "g20_n256", "g9_n35_odd", "g18_n50", "g1_n48"])
def test_device_particle_precompute(name):
    """sum_RefMap / sumsquare_RefMap (same float summation order: bitwise) and the particle r2c on the device against
    the oracle's precalculate (map.cpp:557-630, bioem.cpp:2087-2107) at every BASELINE image size (128, 224, 256),
    the mixed-radix 200, an odd size and two small even ones; then the whole path from those device spectra."""
    case, S = setup_for(name)
    E = make_engine(S, 1, real_space_particles=True)
    spec, s, s2 = E.debug_particles()
    assert np.array_equal(s, S.sumRef) and np.array_equal(s2, S.sumsqRef)
    assert np.abs(spec - S.refFFT).max() <= 2e-6 * np.abs(S.refFFT).max()
    _, pmap, _ = run_native(E, S)
    want, _ = S.run(1)
    assert_same_posterior(S, pmap, want)
    E.close()


def test_device_particle_precompute_odd_size_above_35_and_full_stack():
    """The same chain on synthetic stacks the goldens do not hold: odd sizes above 35 (75, 127, 225) and all 1 000
    particles of the BASELINE config-2 stack (224^2) -- every particle, not a slice."""
    from bioem_amd.synthetic import Workload
    for N, nP in ((75, 5), (127, 4), (225, 3), (224, 1000)):
        W = Workload(N=N, nP=nP, nOrient=4, nEnv=1, npts=200)
        try:
            assert_device_particles_match(W.engine, W.maps, list(range(nP)))
        finally:
            W.engine.close()


def test_write_prob_angles():
    case, S = setup_for("g4_n32_angles")
    for algo in case["algos"]:
        E = make_engine(S, algo)
        _, pmap, pang = run_native(E, S)
        wm, wa = S.run(algo)
        assert_same_posterior(S, pmap, wm)
        la = np.log(pang["forAngles"]) + pang["ConstAngle"]
        lb = np.log(wa["forAngles"]) + wa["ConstAngle"]
        assert np.abs(la - lb).max() <= 1e-3
        rows = orc.ang_prob_rows(S, pmap, pang)
        gold = iof.parse_ang_prob(os.path.join(case["dir"], "ANG_PROB_algo%d" % algo))
        for m in gold:
            for g, r in zip(gold[m], rows[m]):
                assert g["angles"] == [float("%.4f" % v) for v in S.angles[r["orient"]]]
                assert abs(g["logp"] - r["logp"]) <= 5e-3
        E.close()


def make_shard_engine(S, algo, o0, o1):
    import bioem_amd.engine as eng
    E = eng.Engine(pd_of(S), S.nMaps, S.nAngles, S.nCTF, algo=algo, device=0, shard=(o0, o1))
    E.upload_particles(S.refFFT, S.sumRef, S.sumsqRef)
    E.upload_ctf(S.refCTF, S.ctfParam)
    E.upload_model(S.points, S.NormDen, S.px, S.P["shiftX"], S.P["shiftY"])
    E.upload_orientations(S.angles, S.isQuat)
    return E


def run_shard(E, o0, o1):
    import bioem_amd.engine as eng
    raw, pmap, _ = eng.new_prob_block(E.nMaps, 0, 0)        # shard handles move the map entries only
    E.start_run(raw)
    E.project_convolve_compare(o0, o1)
    E.finish_run(raw)
    return raw, pmap


@pytest.mark.parametrize("name,nsh", [("g4_n32_angles", 1), ("g4_n32_angles", 3), ("g11_n32_eulerlist", 2),
                                      ("g11_n32_eulerlist", 14)])
def test_sharded_angle_table_and_device_top_k(name, nsh):
    """WRITE_PROB_ANGLES without moving the table: every shard handle keeps the angle entries of ITS orientation block
    on the device ([o1-o0][nMaps] instead of [nAngles][nMaps]), selects its K best orientations per particle there
    (the writer's min-heap rule, bioem.cpp:1251-1286) and the K-way candidate merge must reproduce the K best of the
    unsharded table: the oracle's rows and the reference's ANG_PROB file (g4, g11 incl. one shard per orientation,
    where every shard owns fewer orientations than K)."""
    import bioem_amd.engine as eng
    case, S = setup_for(name)
    K = S.pd.writeAngles
    numconst = orc.logp_constant(S.pd)
    for algo in case["algos"]:
        blocks, lists = [], []
        for g in range(nsh):
            o0, o1 = g * S.nAngles // nsh, (g + 1) * S.nAngles // nsh
            E = make_shard_engine(S, algo, o0, o1)
            raw, _ = run_shard(E, o0, o1)
            blocks.append(raw.copy())
            c = E.topk_angles(K, numconst)
            assert c.shape == (S.nMaps, K)
            owned = ((c["orient"] >= o0) & (c["orient"] < o1)) | (c["orient"] == -1)
            assert owned.all() and (c["orient"] >= 0).sum(axis=1).min() == min(K, o1 - o0)
            if nsh > 1:
                with pytest.raises(RuntimeError, match="outside the range"):
                    E.project_convolve_compare(0, S.nAngles)
            lists.append(c)
            E.close()
        merged = eng.merge_host(blocks, S.nMaps, 0, 0).view(eng.PROB_MAP_DTYPE)
        cand = eng.merge_topk_host(lists)
        wm, wa = S.run(algo)
        assert_same_posterior(S, merged, wm)
        rows = orc.ang_prob_rows(S, wm, wa)
        gold = iof.parse_ang_prob(os.path.join(case["dir"], "ANG_PROB_algo%d" % algo))
        pri = S.P.get("angprior")
        for m in range(S.nMaps):
            assert [r["orient"] for r in rows[m]] == [int(v) for v in cand[m]["orient"]]
            for g, r, c in zip(gold[m], rows[m], cand[m]):
                lp = c["logp"] + (float(pri[c["orient"]]) if pri is not None else 0.0)
                assert abs(lp - r["logp"]) <= 5e-3 and abs(lp - g["logp"]) <= 5e-3
                assert abs(np.log(c["forAngles"]) - g["sep"][0]) <= 5e-3 and abs(c["ConstAngle"] - g["sep"][1]) <= 5e-3
                assert g["angles"] == [float("%.4f" % v) for v in S.angles[c["orient"]][:len(g["angles"])]]


def test_rccl_merge_single_rank_communicator():
    """bioem_hip_merge: the shard merge behind the C ABI over RCCL (ncclCommInitAll + one ncclAllGather, fold on the
    device).  The box has one GPU, so the communicator has one rank: RCCL initialises, the collective runs on the
    engine's stream, the folded block and the K best orientations come back -- equal to what finish_run / topk_angles
    deliver.  Two handles on one device are refused (one GPU per shard)."""
    import torch  # noqa: F401  (first, so that the process holds PyTorch's copy of RCCL and no second one)
    import bioem_amd.engine as eng
    case, S = setup_for("g4_n32_angles")
    K = S.pd.writeAngles
    numconst = orc.logp_constant(S.pd)
    E = make_shard_engine(S, 1, 0, S.nAngles)
    _, pmap = run_shard(E, 0, S.nAngles)
    want_c = E.topk_angles(K, numconst)
    got, got_c = eng.merge_rccl([E], K, numconst)
    assert got.tobytes() == pmap.tobytes()
    assert got_c.tobytes() == want_c.tobytes()
    got2, none = eng.merge_rccl([E])                       # maps only, cached communicator
    assert none is None and got2.tobytes() == pmap.tobytes()
    E2 = make_shard_engine(S, 1, 0, S.nAngles)
    with pytest.raises(RuntimeError, match="one GPU per shard"):
        eng.merge_rccl([E, E2])
    E.close()
    E2.close()


def test_torch_rccl_merge_single_rank_process_group():
    """bench.py's exchange step on the real backend: torch.distributed with backend "nccl" (= RCCL on ROCm), a
    one-rank process group on the box's GPU, all_gather_into_tensor on device tensors inside merge_prob_maps --
    map entries, orientation offset and the K-best candidates come back as the host merge delivers them."""
    import socket
    import torch
    import torch.distributed as dist
    import bioem_amd.engine as eng
    from bioem_amd.dist_merge import merge_prob_maps
    case, S = setup_for("g4_n32_angles")
    K = S.pd.writeAngles
    E = make_shard_engine(S, 1, 0, S.nAngles)
    _, pmap = run_shard(E, 0, S.nAngles)
    cands = E.topk_angles(K, orc.logp_constant(S.pd))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        merged, mc = merge_prob_maps(pmap, torch.device("cuda", 0), orient_offset=7, cands=cands)
    finally:
        dist.destroy_process_group()
    want = pmap.copy()
    want["orient"] += 7
    assert merged.tobytes() == want.tobytes()
    wc = cands.copy()
    wc["orient"] = np.where(wc["orient"] >= 0, wc["orient"] + 7, wc["orient"])
    assert mc.tobytes() == wc.tobytes()
    E.close()


def test_ctf_range_entry_and_split_merge():
    """bioem_hip_project_convolve_compare_ctf: the CTF grid split (used when there are fewer orientations than GPUs).
    Pieces (orientation block x CTF range) with private blocks, merged in serial visiting order == one run, map entries
    and angle table."""
    import bioem_amd.engine as eng
    case, S = setup_for("g4_n32_angles")
    E = make_engine(S, 1)
    _, full, fang = run_native(E, S)
    blocks = []
    cuts = [0, 1, 3, S.nCTF]
    for o0, o1 in ((0, 5), (5, S.nAngles)):
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            raw, _, _ = eng.new_prob_block(S.nMaps, S.nAngles, S.pd.writeAngles)
            E.start_run(raw)
            E.project_convolve_compare_ctf(o0, o1, c0, c1)
            E.finish_run(raw)
            blocks.append(raw.copy())
    merged = eng.merge_host(blocks, S.nMaps, S.nAngles, S.pd.writeAngles)
    mm = merged[:S.nMaps * 40].view(eng.PROB_MAP_DTYPE)
    ma = merged[S.nMaps * 40:].view(eng.PROB_ANGLE_DTYPE).reshape(S.nAngles, S.nMaps)
    for a, b in zip(mm, full):
        assert abs(S.final_logp(a) - S.final_logp(b)) <= 1e-9 * abs(S.final_logp(b))
        assert (a["orient"], a["conv"], a["cent_x"], a["cent_y"]) == (b["orient"], b["conv"], b["cent_x"], b["cent_y"])
    la = np.log(ma["forAngles"]) + ma["ConstAngle"]
    lb = np.log(fang["forAngles"]) + fang["ConstAngle"]
    assert np.abs(la - lb).max() <= 1e-9 * np.abs(lb).max()
    with pytest.raises(RuntimeError, match="range invalid"):
        E.project_convolve_compare_ctf(0, 1, 2, 2)
    E.close()


def test_orientation_shards_merge_to_unsharded_result():
    """(e) multi-GPU semantics on one GPU: k orientation blocks with private probability blocks, merged by the
    log-sum-exp rule == single run."""
    import bioem_amd.engine as eng
    case, S = setup_for("g2_n128")
    E = make_engine(S, 1)
    raw_full, full, _ = run_native(E, S)
    blocks = []
    nsh = 3
    for g in range(nsh):
        o0, o1 = g * S.nAngles // nsh, (g + 1) * S.nAngles // nsh
        raw, _, _ = run_native(E, S, o0, o1)
        blocks.append(raw.copy())
    merged = eng.merge_host(blocks, S.nMaps, S.nAngles, 0).view(eng.PROB_MAP_DTYPE)
    for a, b in zip(merged, full):
        assert abs(S.final_logp(a) - S.final_logp(b)) <= 1e-9 * abs(S.final_logp(b))
        assert (a["orient"], a["conv"], a["cent_x"], a["cent_y"]) == (b["orient"], b["conv"], b["cent_x"], b["cent_y"])
    E.close()


def test_edge_cases_single_particle_zero_displacement_ragged_batches():
    """nMaps = 1, maxD = 0 (one displacement), nCTF not a multiple of the 4-wave block, orientation count not a
    multiple of the batch."""
    case, S0 = setup_for("g10_n64")
    P = dict(case["P"])
    P["maxD"], P["gridSpace"] = 0, 1
    P["nEnv"], P["nPhase"] = 3, 1
    S = orc.Setup(P, case["model"], case["maps"][:1], case["orient_lines"][:7])
    for algo in (1, 2):
        E = make_engine(S, algo)
        _, pmap, _ = run_native(E, S)
        want, _ = S.run(algo)
        assert_same_posterior(S, pmap, want)
        E.close()
    # large window on the fast path's second instantiation (maxD > 10) and a coarse grid
    P = dict(case["P"])
    P["maxD"], P["gridSpace"] = 13, 3
    S = orc.Setup(P, case["model"], case["maps"][:3], case["orient_lines"][:5])
    for algo in (1, 2):
        E = make_engine(S, algo)
        assert E.fast_path
        _, pmap, _ = run_native(E, S)
        want, _ = S.run(algo)
        assert_same_posterior(S, pmap, want)
        E.close()


def test_invalid_configuration_is_rejected():
    import bioem_amd.engine as eng
    case, S = setup_for("g3_n32_trace")
    pd = pd_of(S)
    pd.maxDisplaceCenter = 40           # >= N/2
    with pytest.raises(RuntimeError, match="invalid configuration"):
        eng.Engine(pd, 2, 4, 2)
    E = make_engine(S, 1)
    with pytest.raises(RuntimeError, match="range invalid"):
        E.project_convolve_compare(0, S.nAngles + 1)
    E.close()


CLI_CASES = ["g10_n64", "g1_n48", "g7_n224", "g19_n200", "g9_n35_odd", "g4_n32_angles", "g5_n32_psf", "g11_n32_eulerlist", "g12_n32_misc",
             "g13_n32_psf_writectf", "g14_n32_mrc", "g15_n32_mrc_nonorm", "g16_n40", "g17_n36", "g18_n50",
             "g20_n256", "g21_n64_wide20", "g22_n128_wide40", "g23_n128_tutorial", "g24_n32_pdb", "g25_n32_modelmrc",
             "g26_n32_multimrc"]


# (case, orientation shards): BIOEM_SHARDS > 1 runs the CLI's multi-GPU control flow (one engine context and host
# thread per shard, private probability blocks, host log-sum-exp merge) with all shards on the one GPU of the box
# shards > orientations: the (orientation, CTF) pairs are split instead (g3: 4 x 2, g11: 14 x 4 with WRITE_PROB_ANGLES)
CLI_RUNS = [(c, 1) for c in CLI_CASES] + [("g10_n64", 3), ("g4_n32_angles", 2), ("g11_n32_eulerlist", 5),
                                          ("g2_n128", 4), ("g3_n32_trace", 6), ("g11_n32_eulerlist", 20),
                                          ("g4_n32_angles", 24)]


@pytest.mark.parametrize("name,shards", CLI_RUNS)
def test_cli_end_to_end_against_reference_outputs(name, shards, tmp_path):
    """The drop-in CLI (--Modelfile/--Particlesfile/--Inputfile[/--ReadOrientation][/--ReadMRC [--ReadMultipleMRC]]
    [/--ReadPDB | --ReadModelMRC]) on the golden
    inputs, with the same files, options and environment the reference was run with: Output_Probabilities /
    ANG_PROB parsed and compared with the reference's own files; the header block must be byte-identical."""
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"
    case, S = setup_for(name)
    d = tmp_path
    cmd = [exe, "--Inputfile", os.path.join(case["dir"], "param.txt"), "--OutputFile", "out.txt"] + \
        write_case_inputs(case, d)
    for algo in case["algos"]:
        env = dict(os.environ, BIOEM_ALGO=str(algo), BIOEM_GPUS="1", BIOEM_SHARDS=str(shards))
        env.update(case["env"])
        r = subprocess.run(cmd, cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        text = open(d / "out.txt").read()
        gold_text = golden_output(case, algo)
        assert text.split("\n\n")[0] == gold_text.split("\n\n")[0]          # header block byte-identical
        gold = iof.parse_output_probabilities(gold_text)
        mine = iof.parse_output_probabilities(text)
        assert len(gold) == len(mine)
        for g, m in zip(gold, mine):
            assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
            assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])
            assert abs(g["norm"] - m["norm"]) <= 2e-4 and abs(g["mu"] - m["mu"]) <= 2e-4
        gl = [ln for ln in gold_text.split("\n") if "CTFMaxParam" in ln]
        ml = [ln for ln in text.split("\n") if "CTFMaxParam" in ln]
        assert gl == ml                                                        # WRITE_CTF_PARAM lines
        if S.pd.writeAngles:
            ga = iof.parse_ang_prob(os.path.join(case["dir"], "ANG_PROB_algo%d" % algo))
            ma = iof.parse_ang_prob(str(d / "ANG_PROB"))
            assert sorted(ga) == sorted(ma)
            for m_ in ga:
                assert len(ga[m_]) == len(ma[m_])
                for g, m in zip(ga[m_], ma[m_]):
                    assert g["angles"] == m["angles"] and abs(g["logp"] - m["logp"]) <= 5e-3
                    assert len(g["sep"]) == len(m["sep"])


@pytest.mark.parametrize("name", ["g4_n32_angles", "g10_n64"])
def test_cli_merges_over_rccl(name, tmp_path):
    """The CLI's multi-GPU exchange step (bioem_hip_merge: RCCL all-gather + device fold + K-best candidates) with the
    one-rank communicator a one-GPU box allows (BIOEM_FORCE_RCCL=1): outputs equal to the reference's files."""
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    case, S = setup_for(name)
    cmd = [exe, "--Inputfile", os.path.join(case["dir"], "param.txt"), "--OutputFile", "out.txt"] + \
        write_case_inputs(case, tmp_path)
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, BIOEM_GPUS="1", BIOEM_FORCE_RCCL="1",
                                                        BIOEM_DEBUG_OUTPUT="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "merge RCCL" in r.stdout
    gold = iof.parse_output_probabilities(golden_output(case, 1))
    mine = iof.parse_output_probabilities(open(tmp_path / "out.txt").read())
    for g, m in zip(gold, mine):
        assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
        assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])
    if S.pd.writeAngles:
        ga = iof.parse_ang_prob(os.path.join(case["dir"], "ANG_PROB_algo1"))
        ma = iof.parse_ang_prob(str(tmp_path / "ANG_PROB"))
        for m_ in ga:
            assert [g["angles"] for g in ga[m_]] == [m["angles"] for m in ma[m_]]
            for g, m in zip(ga[m_], ma[m_]):
                assert abs(g["logp"] - m["logp"]) <= 5e-3


def test_cli_accepts_the_reference_performance_knobs(tmp_path):
    """A job script written for the reference may set its CPU/GPU balancing and CUDA tuning knobs
    (bioem.cpp:99-135, bioem_cuda.cu:216-222): they are read, reported as having no effect, and change nothing."""
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    case, S = setup_for("g10_n64")
    cmd = [exe, "--Inputfile", os.path.join(case["dir"], "param.txt"), "--OutputFile", "out.txt"] + \
        write_case_inputs(case, tmp_path)
    knobs = {"GPU": "1", "GPUWORKLOAD": "60", "GPUASYNC": "0", "GPUDUALSTREAM": "0", "BIOEM_CUDA_THREAD_COUNT": "128",
             "BIOEM_PROJ_CONV_AT_ONCE": "4", "OMP_NUM_THREADS": "7"}
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, BIOEM_GPUS="1", **knobs), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    for k, v in knobs.items():
        if k != "GPU":
            assert "Note - %s=%s accepted, no effect" % (k, v) in r.stdout
    with_knobs = open(tmp_path / "out.txt").read()
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, BIOEM_GPUS="1", GPU="0"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "GPU=0 accepted, no effect" in r.stdout
    assert open(tmp_path / "out.txt").read() == with_knobs
    gold = iof.parse_output_probabilities(golden_output(case, 1))
    mine = iof.parse_output_probabilities(with_knobs)
    for g, m in zip(gold, mine):
        assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
        assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])


@pytest.mark.parametrize("name,nO", [("g2_n128", 24), ("g7_n224", 8)])
@pytest.mark.parametrize("algo", [1, 2])
def test_psf_mode_at_128_and_224_against_oracle(name, nO, algo, tmp_path):
    """USE_PSF (param.cpp:1466-1535: real-space kernel on the wrapped radius, r2c; calc_logpro's PSF prior,
    bioem_algorithm.h:59-66) at the BASELINE image sizes: the golden PSF cases are 32^2.  Model, particles and
    orientations of a golden case with its CTF lines replaced by a PSF grid; device engine against the oracle."""
    case, _ = setup_for(name)
    txt = open(os.path.join(case["dir"], "param.txt")).read().split("\n")
    txt = [ln for ln in txt if ln and not ln.startswith("CTF_")]
    txt += ["USE_PSF", "PSF_AMPLITUDE 0.1 0.3 2", "PSF_ENVELOPE 0.02 0.08 2", "PSF_PHASE 0.01 0.05 1"]
    pf = tmp_path / "param_psf.txt"
    pf.write_text("\n".join(txt) + "\n")
    P = orc.parse_param_file(str(pf))
    assert P["usepsf"]
    S = orc.Setup(P, case["model"], case["maps"], case["orient_lines"], debug_break=nO)
    assert int(S.pd.tousepsf) == 1 and S.nCTF == 4
    E = make_engine(S, algo)
    _, pmap, _ = run_native(E, S)
    want, _ = S.run(algo)
    assert_same_posterior(S, pmap, want)
    E.close()


def test_cli_debug_output_prints_the_reference_phase_report(tmp_path):
    """BIOEM_DEBUG_OUTPUT: the reference's built-in profile (timer.cpp:156-165, bioem.cpp:769-889) -- the four SUMMARY
    lines at level 1, the per-batch "Time Projection / Convolution / Comparison" lines at level 2, in its formats; the
    output file does not change."""
    import re
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    case, S = setup_for("g10_n64")
    cmd = [exe, "--Inputfile", os.path.join(case["dir"], "param.txt"), "--OutputFile", "out.txt"] + \
        write_case_inputs(case, tmp_path)
    outs = {}
    for level in ("0", "1", "2"):
        r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, BIOEM_GPUS="1", BIOEM_DEBUG_OUTPUT=level),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        outs[level] = (r.stdout, open(tmp_path / "out.txt").read())
    assert outs["0"][1] == outs["1"][1] == outs["2"][1]
    assert "SUMMARY" not in outs["0"][0]
    summary = re.compile(r"^SUMMARY -> (Total time of projection|Projection|Convolution|Comparison): Total \d+\.\d{6} sec; "
                         r"Mean \d+\.\d{6} sec; Std\.Dev\. \d+\.\d{6} \(rank 0\)$", re.M)
    for level in ("1", "2"):
        names = [m.group(1) for m in summary.finditer(outs[level][0])]
        assert names == ["Total time of projection", "Projection", "Convolution", "Comparison"], outs[level][0][-1500:]
    assert "Time Projection" not in outs["1"][0]
    two = outs["2"][0]
    assert re.search(r"^\tTime Projection 0-\d+: \d+\.\d{6} \(rank 0\)$", two, re.M)
    assert re.search(r"^\t\tTime Convolution 0-\d+ 0-\d+: \d+\.\d{6} \(rank 0\)$", two, re.M)
    assert re.search(r"^\t\tTime Comparison 0-\d+ 0-\d+: \d+\.\d{6} sec \(rank 0\)$", two, re.M)


def test_phase_records_cover_every_batch_of_a_pass():
    import bioem_amd.engine as eng
    case, S = setup_for("g10_n64")
    E = make_engine(S, 1)
    E.set_phase_timing(True)
    raw, pmap, _ = eng.new_prob_block(S.nMaps, S.nAngles, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    rec = E.phase_records()
    assert len(rec) >= 3 and set(rec["phase"]) == {0, 1, 2} and (rec["seconds"] > 0).all()
    for ph in (0, 1, 2):                 # the batches of each phase tile [0, nAngles)
        r = rec[rec["phase"] == ph]
        assert r["iOrientBegin"][0] == 0 and r["iOrientEnd"][-1] == S.nAngles
        assert (r["iOrientBegin"][1:] == r["iOrientEnd"][:-1]).all()
    assert len(E.phase_records()) == 0   # handed over once
    E.close()


REF_HIP = os.path.join(ROOT, "oracle", "_ref", "bioEM_ref_hip")


@pytest.mark.skipif(not os.path.exists(REF_HIP), reason="oracle/_ref/bioEM_ref_hip is not on this box (`make -C oracle "
                    "ref_hip` builds it where /root/reference exists; it travels as test infrastructure)")
@pytest.mark.parametrize("name", ["g10_n64", "g4_n32_angles", "g2_n128", "g7_n224", "g22_n128_wide40"])
def test_reference_binary_drives_this_build(name, tmp_path):
    """The compiled drop-in against THIS build of libbioem_hip.so (the committed plugin outputs record one past run):
    the unmodified reference sources + oracle/ref_plugin (`make -C oracle ref_hip`), GPU=1, the reference's own run()
    loop calling the engine through the compareRefMaps virtual (bioem.cpp:853) -- outputs against the reference CPU
    path's committed files."""
    case, S = setup_for(name)
    args = write_case_inputs(case, tmp_path)
    for algo in case["algos"]:
        env = dict(os.environ, OMP_NUM_THREADS="1", BIOEM_ALGO=str(algo), BIOEM_DEBUG_OUTPUT="0", GPU="1")
        if algo == 2:
            env["BIOEM_PROJ_CONV_AT_ONCE"] = "3"
        env.update(case["env"])
        r = subprocess.run([REF_HIP, "--Inputfile", os.path.join(case["dir"], "param.txt"), "--OutputFile", "out.txt"]
                           + args, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:]
        gold = iof.parse_output_probabilities(golden_output(case, algo))
        mine = iof.parse_output_probabilities(open(tmp_path / "out.txt").read())
        assert len(gold) == len(mine) > 0
        for g, m in zip(gold, mine):
            assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
            assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])
        if S.pd.writeAngles:
            ga = iof.parse_ang_prob(os.path.join(case["dir"], "ANG_PROB_algo%d" % algo))
            ma = iof.parse_ang_prob(str(tmp_path / "ANG_PROB"))
            for m_ in ga:
                assert [g["angles"] for g in ga[m_]] == [m["angles"] for m in ma[m_]]


def test_cli_error_behaviour(tmp_path):
    """Errors print 'Error - ...' and exit 1 like the reference's myError (defs.h:18-26)."""
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    r = subprocess.run([exe, "--Modelfile", "nope", "--Particlesfile", "nope", "--Inputfile", "/nonexistent"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 1 and "Error - Opening file" in r.stdout


# ------------------------------------------------------------------------------------------------------
# full benchmark size (BASELINE config 2): size-independent properties + oracle on a slice
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_workload():
    from bioem_amd.synthetic import Workload
    W = Workload(N=224, nP=1000, nOrient=4608, nEnv=5)    # BASELINE config 2 at its own size
    yield W
    W.engine.close()


def run_workload(W, o0, o1):
    import bioem_amd.engine as eng
    raw, pmap, _ = eng.new_prob_block(W.nP, W.nOrient, 0)
    W.engine.start_run(raw)
    W.engine.project_convolve_compare(o0, o1)
    W.engine.finish_run(raw)
    return raw, pmap


def test_full_size_sharding_invariance_and_planted_truth(full_workload):
    import bioem_amd.engine as eng
    W = full_workload
    raw, full = run_workload(W, 0, W.nOrient)
    assert np.all(np.isfinite(full["Total"])) and np.all(full["Total"] >= 1.0)
    parts = [run_workload(W, a, b)[0].copy() for a, b in [(0, 1700), (1700, 1701), (1701, W.nOrient)]]
    merged = eng.merge_host(parts, W.nP, W.nOrient, 0).view(eng.PROB_MAP_DTYPE)
    lf = np.log(full["Total"]) + full["Constoadd"]
    lm = np.log(merged["Total"]) + merged["Constoadd"]
    assert np.abs(lf - lm).max() <= 1e-9 * np.abs(lf).max()
    for k in ("orient", "conv", "cent_x", "cent_y"):
        assert np.array_equal(full[k], merged[k])
    # idempotence: the same pass twice gives bit-identical posteriors (no atomics / races on the hot path)
    raw2, again = run_workload(W, 0, W.nOrient)
    assert raw.tobytes() == raw2.tobytes()
    # planted truth: particle p was rendered from orientation (7919 p) mod nOrient; at SNR 0.05 the maximum
    # posterior orientation recovers it for the large majority of particles
    truth = (7919 * np.arange(W.nP)) % W.nOrient
    assert np.mean(full["orient"] == truth) > 0.9


def oracle_particle_inputs(maps, sel):
    """What PreCalculateMapsFFT / precalculate hand to the compare path (map.cpp:557-630, bioem.cpp:2087-2107) for the
    particles `sel`, computed by the ORACLE from the real-space maps: r2c spectra and the two sequential float sums."""
    rsel = np.stack([orc.fft2_r2c(maps[p]) for p in sel])
    sums = [orc.map_sums(maps[p]) for p in sel]
    return (np.ascontiguousarray(rsel), np.array([s for s, _ in sums], dtype=np.float32),
            np.array([s2 for _, s2 in sums], dtype=np.float32))


def assert_device_particles_match(E, maps, sel):
    """The device particle chain of bioem_hip_upload_particle_maps (k_map_sums, k_dft_rows/cols, k_reorder) against
    the oracle's precalculate on the same maps: sums bitwise (same summation order), spectra to float rounding."""
    spec, s, s2 = E.debug_particles()
    rsel, ssel, s2sel = oracle_particle_inputs(maps, sel)
    assert np.array_equal(s[sel], ssel) and np.array_equal(s2[sel], s2sel)
    assert np.abs(spec[sel] - rsel).max() <= 2e-6 * np.abs(rsel).max()
    return rsel, ssel, s2sel


def oracle_on_workload(W, sel, nO, algo=1, angles=False, engine=None, maps=None):
    """orientations [0, nO) x all CTFs x the particles `sel` of a synthetic workload through the CPU oracle.  The
    oracle computes its own particle spectra and sums from the real-space maps (`maps`, default W.maps), so the device
    particle transform is NOT on both sides; the engine's copies are asserted against them on the way.  angles=True
    also returns the oracle's angle table [nOrient][len(sel)]."""
    import ctypes as C
    rsel, ssel, s2sel = assert_device_particles_match(engine or W.engine, W.maps if maps is None else maps, sel)
    nsel = len(sel)
    pd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(pd, f, getattr(W.pd, f))
    pts = np.zeros(len(W.points), dtype=orc.POINT_DTYPE)
    for k in ("pos", "radius", "density"):
        pts[k] = W.points[k]
    want = np.zeros(nsel, dtype=orc.PROB_MAP_DTYPE)
    wang = np.zeros((W.nOrient, nsel), dtype=orc.PROB_ANGLE_DTYPE) if angles else None
    L = orc.lib()
    L.orc_init_prob(nsel, W.nOrient, int(pd.writeAngles) if angles else 0, want.ctypes.data,
                    wang.ctypes.data if angles else None)
    if not angles:
        pd.writeAngles = 0
    L.orc_run(C.byref(pd), algo, pts.ctypes.data, len(pts), W.NormDen, W.angles.ctypes.data, W.nOrient, 1, W.px, 0,
              0, W.nCTF, W.refCTF.ctypes.data, W.ctfParam.ctypes.data, nsel, rsel.ctypes.data, ssel.ctypes.data,
              s2sel.ctypes.data, 0, nO, want.ctypes.data, wang.ctypes.data if angles else None)
    if angles:
        return want, orc.logp_constant(pd), wang
    return want, orc.logp_constant(pd)


def assert_workload_matches(got, want, const, sel):
    for i, p in enumerate(sel):
        la = np.log(got[p]["Total"]) + got[p]["Constoadd"] + const
        lb = np.log(want[i]["Total"]) + want[i]["Constoadd"] + const
        # north_star tolerance (1e-4 relative) and, tighter, an absolute bound: 2e-2 or two float spacings of log P --
        # the reference narrows logpro to float (bioem_algorithm.h:84), so one rounding flip moves log P by a spacing
        assert abs(la - lb) <= REL_TOL * abs(lb)
        assert abs(la - lb) <= max(ABS_TOL, 2.0 * float(np.spacing(np.float32(abs(lb)))))
        assert (got[p]["orient"], got[p]["conv"], got[p]["cent_x"], got[p]["cent_y"]) == \
               (want[i]["orient"], want[i]["conv"], want[i]["cent_x"], want[i]["cent_y"])


PREP_SHAPES = {
    # name: (N, orientations, envelopes, defoci) -- what the preparation kernels see: CTFs per block of k_convolve_sums
    # (4 x <= 4, 3 x 5, 3 x 6, several groups of six), orientation counts that do not fill the last block, an odd size
    "ctf1": (64, 5, 1, 1), "ctf3": (64, 7, 3, 1), "ctf4": (96, 6, 4, 1), "ctf5": (64, 4, 5, 1), "ctf6": (64, 5, 6, 1),
    "ctf7_two_groups": (64, 4, 7, 1), "ctf13_three_groups": (80, 3, 13, 1), "ctf10_defocus": (64, 4, 5, 2),
    "odd75": (75, 5, 5, 1), "one_orientation": (64, 1, 5, 1),
}


@pytest.mark.parametrize("name", sorted(PREP_SHAPES) + ["stretching_quaternions", "model_beyond_the_box"])
def test_preparation_kernels_against_oracle(name):
    """Projection (k_project_box; the band kernel where the model leaves the box or the quaternions are not of unit
    length), the boxed r2c and k_convolve_sums<R, NC> in every block shape, through the whole path against the oracle."""
    from bioem_amd.synthetic import Workload
    N, nO, nEnv, nDef = PREP_SHAPES.get(name, (128 if name == "model_beyond_the_box" else 64, 3, 2, 1))
    W = Workload(N=N, nP=3, nOrient=nO, nEnv=nEnv, nDefocus=nDef, npts=150, render=False)
    try:
        E = W.engine
        if name == "stretching_quaternions":     # the reference's matrix is no rotation then (bioem.cpp:1632-1646)
            W.angles = (W.angles * np.float32(1.07)).astype(np.float32)
            E.upload_orientations(W.angles, True)
        if name == "model_beyond_the_box":       # three times the extent: the box would be the whole map
            W.points["pos"] *= np.float32(3.0)
            E.upload_model(W.points, W.NormDen, W.px)
        W.maps = W.render_particles(0.05)
        E.upload_particle_maps(W.maps)
        sel = [0, 1, 2]
        want, const = oracle_on_workload(W, sel, nO, 1)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


@pytest.mark.parametrize("px", [0.9, 0.5, 3.6])
def test_projection_footprints_of_other_widths_against_oracle(px):
    """k_project_stamps / k_project_box with sphere footprints of 9 and 15 pixels (pixel sizes 0.9 and 0.5 A for radii of
    2.25...3.4 A: the footprint column is fetched in two and three groups of five entries) and with every sphere a
    single pixel (3.6 A: radius <= pixel size, bioem.cpp:1700-1712), through the whole path against the oracle."""
    from bioem_amd.synthetic import Workload
    W = Workload(N=96, nP=3, nOrient=5, nEnv=3, px=px, npts=150)
    try:
        sel = [0, 1, 2]
        want, const = oracle_on_workload(W, sel, 5, 1)
        _, got = run_workload(W, 0, 5)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


def test_full_size_slice_against_oracle(full_workload):
    """224^2, all 5 CTFs, 6 orientations x 8 particles of the benchmark workload through the CPU oracle."""
    W = full_workload
    sel = [0, 1, 2, 3, 500, 501, 998, 999]
    nO = 6
    want, const = oracle_on_workload(W, sel, nO)
    _, got = run_workload(W, 0, nO)
    assert_workload_matches(got, want, const, sel)


@pytest.mark.parametrize("N,nP,nEnv,nDef,maxD", [(224, 1000, 5, 1, 10),     # config 2's stack and CTF grid
                                                 (224, 2000, 5, 2, 10),     # config 3's ten CTFs
                                                 (256, 400, 2, 2, 10),      # config 5's image size (Nyquist split)
                                                 (224, 200, 2, 1, 20)])     # 41-row window (k_compare_fastm2)
def test_algo2_at_baseline_sizes_against_oracle(N, nP, nEnv, nDef, maxD):
    """BIOEM_ALGO=2 (doRefMap_CPU_Parallel / _Reduce, bioem.cpp:1461-1602) at the BASELINE image sizes and particle
    counts -- the full-size checks above run ALGO 1: 6 orientations x all CTFs x 8 particles through the oracle."""
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=nP, nOrient=32, nEnv=nEnv, nDefocus=nDef, maxD=maxD, algo=2)
    try:
        sel = [0, 1, 2, 3, nP // 2, nP // 2 + 1, nP - 2, nP - 1]
        want, const = oracle_on_workload(W, sel, 6, algo=2)
        _, got = run_workload(W, 0, 6)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


# ------------------------------------------------------------------------------------------------------
# BASELINE config 3 at one GPU's share of the particle regime: 10 000 particles (2 GB of spectra, beyond the 256 MB
# Infinity Cache), 2 x 5 CTFs, 224^2; 128 orientations = two batches of the device pipeline
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config3_workload():
    from bioem_amd.synthetic import Workload
    W = Workload(N=224, nP=10000, nOrient=128, nEnv=5, nDefocus=2)
    yield W
    W.engine.close()


def test_config3_share_properties_and_oracle_slice(config3_workload):
    import bioem_amd.engine as eng
    W = config3_workload
    assert W.nCTF == 10 and W.engine.kernel_name == "k_compare_fast"
    raw, full = run_workload(W, 0, W.nOrient)
    assert np.all(np.isfinite(full["Total"])) and np.all(full["Total"] >= 1.0)
    # shard-merge invariance: two orientation blocks with private probability blocks (the per-GPU split of config 3)
    parts = [run_workload(W, a, b)[0].copy() for a, b in [(0, 64), (64, W.nOrient)]]
    merged = eng.merge_host(parts, W.nP, W.nOrient, 0).view(eng.PROB_MAP_DTYPE)
    lf = np.log(full["Total"]) + full["Constoadd"]
    lm = np.log(merged["Total"]) + merged["Constoadd"]
    assert np.abs(lf - lm).max() <= 1e-9 * np.abs(lf).max()
    for k in ("orient", "conv", "cent_x", "cent_y"):
        assert np.array_equal(full[k], merged[k])
    # bit-identical rerun (no atomics / races on the hot path at 40 000 resident blocks)
    raw2, _ = run_workload(W, 0, W.nOrient)
    assert raw.tobytes() == raw2.tobytes()
    # planted truth: particle p = orientation (7919 p) mod 128, CTF p mod 10
    truth_o = (7919 * np.arange(W.nP)) % W.nOrient
    assert np.mean(full["orient"] == truth_o) > 0.9
    assert np.mean(full["conv"] == np.arange(W.nP) % W.nCTF) > 0.5
    # the CPU oracle on a slice: 8 particles from both ends and the middle of the stack x 6 orientations x 10 CTFs
    sel = [0, 1, 2, 4999, 5000, 9997, 9998, 9999]
    want, const = oracle_on_workload(W, sel, 6)
    _, got = run_workload(W, 0, 6)
    assert_workload_matches(got, want, const, sel)


# ------------------------------------------------------------------------------------------------------
# BASELINE config 5 shape: 256^2 particles delivered by the MRC reader (--ReadMRC --ReadMultipleMRC path of the
# host layer), 1 000 particles x 2 304 orientations, WRITE_PROB_ANGLES, two orientation shards with sharded angle
# tables and device top-K
# ------------------------------------------------------------------------------------------------------
def test_config5_shape_two_shards_device_top_k(tmp_path):
    import bioem_amd.engine as eng
    from bioem_amd import hostlib
    from bioem_amd.synthetic import Workload
    from golden_util import write_mrc_stack
    K, nO, nP, N = 10, 2304, 1000, 256
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=2, nDefocus=2, write_angles=K)        # one shard handle over [0, nO)
    assert W.nCTF == 4 and W.engine.shard == (0, nO)
    # the particle stack as raw counts in two MRC stacks + list file; the reader transposes and z-scores
    rawcounts = (3.0 * np.transpose(W.maps, (0, 2, 1)) + 7.0).astype(np.float32)
    write_mrc_stack(str(tmp_path / "a.mrc"), rawcounts[:400])
    write_mrc_stack(str(tmp_path / "b.mrc"), rawcounts[400:])
    with open(tmp_path / "list.txt", "w") as f:
        f.write(str(tmp_path / "a.mrc") + "\n" + str(tmp_path / "b.mrc") + "\n")
    maps = hostlib.read_particles(str(tmp_path / "list.txt"), N, mode=2, cap=nP)
    # (the reader's mean / variance are sequential float sums over 65 536 pixels, map.cpp:831-845: ~5e-4 off)
    assert maps.shape == (nP, N, N) and np.abs(maps - W.maps).max() <= 3e-3
    numconst = orc.logp_constant(W.pd)

    def shard(o0, o1):
        E = eng.Engine(W.pd, nP, nO, W.nCTF, algo=1, device=0, shard=(o0, o1))
        E.upload_particle_maps(maps)
        E.upload_ctf(W.refCTF, W.ctfParam)
        E.upload_model(W.points, W.NormDen, W.px)
        E.upload_orientations(W.angles, True)
        raw, pmap = run_shard(E, o0, o1)
        return E, raw.copy(), E.topk_angles(K, numconst)

    Ea, rawa, ca = shard(0, nO // 2)
    Eb, rawb, cb = shard(nO // 2, nO)
    E1, raw1, c1 = shard(0, nO)
    one = raw1.view(eng.PROB_MAP_DTYPE)
    merged = eng.merge_host([rawa, rawb], nP, 0, 0).view(eng.PROB_MAP_DTYPE)
    la = np.log(one["Total"]) + one["Constoadd"]
    lb = np.log(merged["Total"]) + merged["Constoadd"]
    assert np.abs(la - lb).max() <= 1e-9 * np.abs(la).max()
    for k in ("orient", "conv", "cent_x", "cent_y"):
        assert np.array_equal(one[k], merged[k])
    cm = eng.merge_topk_host([ca, cb])
    assert np.array_equal(cm["orient"], c1["orient"])           # K best of the union == K best of the whole table
    assert np.abs(cm["logp"] - c1["logp"]).max() <= 1e-9 * np.abs(c1["logp"]).max()
    assert np.all(np.diff(c1["logp"], axis=1) <= 0)             # best first
    truth = (7919 * np.arange(nP)) % nO
    assert np.mean(c1["orient"][:, 0] == truth) > 0.9           # the planted orientation leads the list
    # oracle on a slice: 8 particles x the first 12 orientations, K best of those 12
    sel = [0, 1, 2, 3, 500, 501, 998, 999]
    for E in (Ea, Eb):
        E.close()
    Es = eng.Engine(W.pd, nP, nO, W.nCTF, algo=1, device=0, shard=(0, 12))
    Es.upload_particle_maps(maps)
    Es.upload_ctf(W.refCTF, W.ctfParam)
    Es.upload_model(W.points, W.NormDen, W.px)
    Es.upload_orientations(W.angles, True)
    _, got = run_shard(Es, 0, 12)
    cs = Es.topk_angles(K, numconst)
    want, const, wang = oracle_on_workload(W, sel, 12, angles=True, engine=Es, maps=maps)
    assert_workload_matches(got, want, const, sel)
    import heapq
    for i, p in enumerate(sel):
        q = []
        for io in range(12):
            pa = wang[io, i]
            heapq.heappush(q, (float(np.log(pa["forAngles"]) + pa["ConstAngle"] + numconst), io))
        best = sorted(q, reverse=True)[:K]
        assert [io for _, io in best] == [int(v) for v in cs[p]["orient"]]
        for (lp, _), c in zip(best, cs[p]):     # same bound as the particle entries: 2e-2 or two float spacings of log P
            assert abs(lp - c["logp"]) <= max(ABS_TOL, 2.0 * float(np.spacing(np.float32(abs(lp)))))
    Es.close()
    E1.close()
    W.engine.close()


# image sizes by the register-FFT length R the comparison kernel picks (N = N1 * R: the power-of-two part of N up to
# 32, or a 2/3/5-smooth divisor up to 30 when that part is 2 or 4); odd N and windows beyond +-15 rows -> the
# generic pruned-DFT kernel
@pytest.mark.parametrize("N,maxD,grid,fast", [(40, 10, 1, 1), (72, 7, 1, 1), (200, 10, 1, 1), (80, 12, 1, 1),
                                              (48, 15, 1, 1), (96, 10, 2, 1), (160, 10, 1, 1), (256, 10, 1, 1),
                                              (100, 10, 1, 1), (36, 5, 1, 1), (180, 10, 1, 1), (250, 10, 1, 1),
                                              (90, 9, 3, 1), (10, 2, 1, 1), (75, 10, 1, 0), (64, 16, 1, 1),
                                              # coarse grids: window rows step by the gcd of the offsets (1..4)
                                              (64, 30, 2, 1), (224, 20, 2, 1), (128, 40, 4, 1), (96, 45, 3, 1),
                                              (64, 9, 2, 1), (100, 25, 5, 0), (64, 31, 2, 0),
                                              # register-FFT lengths: 56 -> 8, 44 -> 4, 34 -> 2 (radix 2); mixed radix
                                              # 42 -> 6, 50 -> 10, 84 -> 12, 36 -> 18, 100 -> 20, 90/180/150 -> 30
                                              (56, 10, 1, 1), (44, 10, 1, 1), (34, 8, 1, 1), (42, 10, 1, 1),
                                              (84, 10, 1, 1), (120, 10, 1, 1), (150, 10, 1, 1), (300, 10, 1, 1),
                                              # 31-row window: R = 16 + half-width T exchange (3 waves per SIMD); with
                                              # the Nyquist split (128) it stays at R = 32
                                              (224, 13, 1, 1), (128, 15, 1, 1), (160, 12, 1, 1), (200, 15, 1, 1),
                                              # ... and the mixed-radix sizes with a length <= 16 (180 -> 12, 150 -> 10,
                                              # 100 -> 10, 300 -> 12, 90 -> 10, 84 -> 12, 42 -> 6) instead of 30 / 20 / 18
                                              (180, 15, 1, 1), (150, 12, 1, 1), (100, 15, 1, 1), (300, 13, 1, 1),
                                              (90, 11, 1, 1), (84, 14, 1, 1), (42, 15, 1, 1), (180, 30, 2, 1),
                                              # wide windows (the reference's tutorial suggests DISPLACE_CENTER 40 1):
                                              # tiles of the 21- / 31-row window on phase-shifted conv spectra
                                              (64, 20, 1, 1), (128, 40, 1, 1), (224, 20, 1, 1), (100, 40, 2, 1),
                                              (64, 31, 1, 1), (96, 16, 1, 1), (256, 25, 1, 1), (75, 20, 1, 0), (225, 40, 1, 0),
                                              (320, 20, 1, 1), (384, 40, 2, 1), (272, 16, 1, 1), (100, 40, 1, 1), (180, 20, 1, 1), (250, 30, 1, 1),
                                              (150, 16, 1, 1), (44, 20, 1, 1), (60, 25, 1, 1),
                                              # odd sizes: k_compare_rows (direct column sums + the fast kernel's back half)
                                              (225, 10, 1, 0), (127, 12, 1, 0), (51, 15, 1, 0), (99, 10, 2, 0),
                                              (33, 4, 1, 0), (129, 20, 2, 0), (9, 2, 1, 0), (125, 40, 1, 0), (75, 16, 1, 0),
                                              # small windows: the 11-row template (rows <= +-5)
                                              (224, 5, 1, 1), (128, 10, 2, 1), (64, 0, 1, 1), (96, 20, 4, 1),
                                              (80, 4, 2, 1), (224, 10, 2, 1),
                                              # ... which the largest sizes run on the 21-row template
                                              (400, 5, 1, 1), (360, 4, 1, 1),
                                              # windows no single kernel covers -> tiles of k_compare_fastm / k_compare_fast
                                              # (Nyquist split beyond +-42 px, 101 rows, images beyond 512 pixels)
                                              (128, 45, 1, 1), (130, 50, 1, 1), (256, 47, 1, 1), (600, 18, 1, 1),
                                              (520, 40, 1, 1), (100, 45, 3, 1)])
@pytest.mark.parametrize("algo", [1, 2])
def test_image_sizes_against_oracle(N, maxD, grid, fast, algo):
    from bioem_amd.synthetic import Workload
    nP, nO = 6, 9                                   # 9 orientations x 2 CTFs = 18 comparisons: ragged last group
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=2, maxD=maxD, grid=grid, algo=algo, npts=300)
    try:
        assert W.engine.fast_path is bool(fast)
        sel = list(range(nP))
        want, const = oracle_on_workload(W, sel, nO, algo)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


# k_compare_generic with a window whose T block does not fit the LDS at once (compare_generic.hpp: the rows pass through in
# groups of whole 16-row chunks): displacement sets off the grid (maxD % grid != 0) and strides beyond 4 with 45...89 rows --
# shapes that bioem_hip_create rejected before the end of round 4 ("exceeds the 160 KiB LDS budget"); an uneven last group,
# odd N, both algorithms
@pytest.mark.parametrize("N,maxD,grid,nP,nO", [(200, 98, 3, 3, 3), (225, 110, 5, 3, 2), (448, 220, 5, 2, 1),
                                               (512, 162, 4, 2, 1)])
@pytest.mark.parametrize("algo", [1, 2])
def test_generic_kernel_windows_beyond_the_lds(N, maxD, grid, nP, nO, algo):
    from bioem_amd.synthetic import Workload
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=1, maxD=maxD, grid=grid, algo=algo, npts=200)
    try:
        assert W.engine.kernel_signature == "k_compare_generic"
        sel = list(range(nP))
        want, const = oracle_on_workload(W, sel, nO, algo)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


# k_compare_fast with a last column block of at most 32 columns: its half-waves share the columns, the low half the first
# ceil(N1 / 2) k1 steps, the high half the rest (compare_fast.hpp).  One block only (60), two (144...190), three (288,
# 300), even and odd N1 (160 = 10 x 16, 144 = 9 x 16, 150 = 15 x 10, 190 = 19 x 10), 11- and 21-row windows, a coarse grid
@pytest.mark.parametrize("N,maxD,grid", [(60, 10, 1), (144, 10, 1), (150, 5, 1), (160, 10, 1), (160, 5, 1), (176, 20, 2),
                                         (190, 10, 1), (288, 10, 1), (300, 5, 1), (138, 9, 1),
                                         # ... and of k_compare_fastm (27 / 31 rows)
                                         (160, 13, 1), (144, 15, 1), (150, 13, 1), (176, 26, 2), (288, 15, 1), (60, 13, 1),
                                         # ... and N / 2 = 32 (mod 64): Nyquist column apart, the 32 columns beyond the
                                         # whole blocks as a split block (planned that way: no unsplit pass to compare)
                                         (192, 10, 1), (192, 5, 1), (192, 20, 2), (64, 10, 1), (64, 5, 1), (320, 10, 1)])
@pytest.mark.parametrize("algo", [1, 2])
def test_split_last_column_block_against_oracle(N, maxD, grid, algo, monkeypatch):
    from bioem_amd.synthetic import Workload
    nP, nO = 5, 6
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=2, maxD=maxD, grid=grid, algo=algo, npts=300)
    try:
        assert W.engine.kernel_signature.startswith(("k_compare_fast<", "k_compare_fastm<"))
        sel = list(range(nP))
        want, const = oracle_on_workload(W, sel, nO, algo)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
        # and the unsplit pass of the same kernel (BIOEM_NO_SPLIT_LAST is read at every launch): the same arg-max tuples
        if N not in (64, 192) and (N, maxD) != (320, 10):
            monkeypatch.setenv("BIOEM_NO_SPLIT_LAST", "1")
            _, plain = run_workload(W, 0, nO)
            assert_workload_matches(plain, want, const, sel)
            assert np.array_equal(got["orient"], plain["orient"]) and np.array_equal(got["cent_x"], plain["cent_x"])
    finally:
        W.engine.close()


# Padded row-pair pitch of the comparison layout (bioem_hip.hip, comparison_pitch: N a multiple of 64 from 192 pixels on,
# plans of the one-wave-per-comparison families): same arithmetic at other addresses -- the probability
# block equals the unpadded layout's (BIOEM_NO_PITCH_PAD=1, read when the handle is created) BIT FOR BIT, through the
# fused convolution (few particles) and the two-kernel one, for 11-, 21-, 27- and 41-row windows, and against the oracle
@pytest.mark.parametrize("N,maxD,nP", [(256, 10, 4), (256, 5, 4), (256, 13, 4), (256, 20, 4), (256, 10, 300), (384, 10, 3),
                                       (192, 10, 4), (192, 5, 4), (320, 10, 3),
                                       # ... and plans without the Nyquist split
                                       (448, 10, 3), (320, 5, 3), (192, 13, 4), (320, 20, 3)])
def test_padded_pitch_equals_the_plain_layout_bit_for_bit(N, maxD, nP, monkeypatch):
    from bioem_amd.synthetic import Workload
    nO = 5
    blocks = []
    for pad in (True, False):
        if not pad:
            monkeypatch.setenv("BIOEM_NO_PITCH_PAD", "1")
        W = Workload(N=N, nP=nP, nOrient=nO, nEnv=2, maxD=maxD, npts=300)
        try:
            raw, got = run_workload(W, 0, nO)
            # (the hooks hand out the reference layout whatever the device layout is)
            blocks.append(raw.tobytes() + W.engine.debug_convolution(nO - 1, 1)[0].tobytes() +
                          W.engine.debug_particles()[0].tobytes())
            if pad and nP <= 4:
                sel = list(range(nP))
                want, const = oracle_on_workload(W, sel, nO, 1)
                assert_workload_matches(got, want, const, sel)
        finally:
            W.engine.close()
    assert blocks[0] == blocks[1]


# k_compare_wide2 (shared column transforms + row FFT) is picked from three 21-row tiles per axis on; forced here for
# every register-FFT length, one and two column blocks, the Nyquist split, row strides 1..3, odd and even row counts
# per wave, windows from +-16 to +-41 px
@pytest.mark.parametrize("N,maxD,grid", [(64, 20, 1), (128, 40, 1), (224, 20, 1), (224, 41, 1), (100, 40, 2), (96, 16, 1),
                                         (256, 25, 1), (180, 20, 1), (250, 30, 1), (150, 16, 1), (44, 20, 1),
                                         (60, 25, 1), (120, 22, 1), (90, 40, 2), (200, 33, 1), (36, 16, 1), (84, 30, 1),
                                         (34, 16, 1), (128, 62, 2),
                                         # three waves per SIMD variant (<= 11 rows per wave, two column blocks, R 16 / 8)
                                         (240, 18, 1), (200, 20, 1), (160, 17, 1), (224, 12, 1), (224, 21, 1),
                                         (208, 44, 2), (224, 24, 1), (200, 25, 1), (160, 26, 1),
                                         # ... with the Nyquist split (256^2, 128^2) and one column block
                                         (256, 16, 1), (256, 20, 1), (128, 20, 1), (128, 30, 1), (120, 25, 1),
                                         (96, 20, 1),
                                         # T block through LDS in two halves (one block per CU otherwise): even / odd halves,
                                         # Nyquist split, mixed radix, row stride 2
                                         (256, 40, 1), (240, 38, 1), (250, 40, 1), (256, 37, 1), (248, 78, 2),
                                         # three column blocks (256 < N <= 384), whole T block and halves, every length
                                         # with such an instantiation, Nyquist split (384)
                                         (320, 40, 1), (288, 25, 1), (272, 40, 1), (300, 30, 1), (360, 40, 1), (280, 27, 1),
                                         (264, 35, 1), (290, 22, 1), (384, 40, 1), (384, 20, 1), (380, 80, 2),
                                         # 22..24 rows per wave over two column blocks
                                         (208, 42, 1), (224, 47, 1), (256, 42, 1), (192, 88, 2),
                                         # four column blocks (384 < N <= 512), at most 11 rows per wave
                                         (448, 20, 1), (512, 20, 1), (400, 18, 1), (512, 16, 1), (432, 42, 2),
                                         # eight waves per comparison (16- / 10-point FFTs, two blocks per CU)
                                         (208, 30, 1), (240, 34, 1), (176, 40, 1), (144, 43, 1), (250, 30, 1), (240, 64, 2),
                                         # ... over four column blocks
                                         (512, 40, 1), (448, 30, 1), (400, 43, 1), (512, 23, 1)])
@pytest.mark.parametrize("algo", [1, 2])
def test_wide2_kernel_against_oracle(N, maxD, grid, algo, monkeypatch):
    from bioem_amd.synthetic import Workload
    monkeypatch.setenv("BIOEM_FORCE_WIDE2", "1")
    nP, nO = 5, 7                                   # 7 orientations x 2 CTFs x 5 particles
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=2, maxD=maxD, grid=grid, algo=algo, npts=300)
    try:
        # (which instantiation a shape runs is pinned by tests/test_selection_table.py; a forced shape whose
        # instantiation is not in the kernel table falls back to its ordinary kernel and is not this test's business)
        if W.engine.kernel_name != "k_compare_wide2":
            pytest.skip("no k_compare_wide2 instantiation for this shape: " + W.engine.kernel_signature)
        sel = list(range(nP))
        want, const = oracle_on_workload(W, sel, nO, algo)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


@pytest.mark.parametrize("N,maxD,grid", [(224, 20, 1), (224, 16, 1), (224, 23, 1), (128, 20, 1), (256, 21, 1), (208, 18, 1),
                                         (64, 16, 1), (96, 22, 1), (160, 19, 1), (336, 17, 1), (512, 20, 1), (240, 23, 1),
                                         # register FFTs of 12 / 10 / 8 points where 16 does not divide N
                                         (180, 17, 1), (300, 20, 1), (200, 20, 1), (250, 16, 1), (248, 23, 1), (88, 18, 1),
                                         # row strides 2 / 3 / 4 (rows 4 / 8 / 2 apart pair up), also with the Nyquist split
                                         (224, 40, 2), (224, 51, 3), (224, 80, 4), (256, 44, 2), (128, 48, 3), (256, 68, 4),
                                         (208, 36, 2)])
@pytest.mark.parametrize("algo", [1, 2])
def test_fastm2_kernel_against_oracle(N, maxD, grid, algo):
    """k_compare_fastm2 (33..47-row windows: rows split over the half-waves, 3 x 3 matrix tiles): every instantiation --
    the Nyquist split (128 / 256 / 512), register FFTs of 16 / 12 / 10 / 8 points, row strides 1..4 --, an odd number of
    sub-transforms (208 = 13 x 16, 240, 336, 200 = 25 x 8 ...: the high half of the last step reads beyond the buffer), a
    partly filled last column pass, the narrowest and the widest window of the family, ALGO 1 / 2 (a stride that does
    not divide maxD gives ALGO 1 an irregular set: that shape is not this kernel's)."""
    from bioem_amd.synthetic import Workload
    nP, nO = 5, 7
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=2, maxD=maxD, grid=grid, algo=algo, npts=300)
    try:
        if maxD % grid == 0:
            assert W.engine.kernel_name == "k_compare_fastm2"
        sel = list(range(nP))
        want, const = oracle_on_workload(W, sel, nO, algo)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


def _random_configs(n, seed, sizes=None):
    """Seeded random (N, maxD, grid, algo, nEnv, nP, nO) tuples over the whole configuration space of the comparison
    kernels: every register-FFT length, the Nyquist split, window templates, row strides, tiles, the generic path."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        N = int(rng.choice([int(rng.integers(8, 140)), int(rng.choice([32, 48, 64, 96, 128, 160, 192, 200, 224, 256]))]))
        if sizes:                                  # (scripts/fuzz_configs.py --sizes: a fuzz of chosen image sizes)
            N = int(rng.choice(sizes))
        grid = int(rng.choice([1, 1, 1, 2, 3, 4, 5]))
        maxD = int(rng.integers(0, max(1, N // 2 - 1)))
        if rng.random() < 0.5:
            maxD = min(maxD, 12 * grid)
        if maxD // grid > 45:                      # keep the oracle's share of the run time small
            continue
        out.append((N, maxD, grid, int(rng.choice([1, 2])), int(rng.choice([1, 2, 3])), int(rng.integers(1, 6)),
                    int(rng.integers(1, 8))))
    return out


@pytest.mark.parametrize("cfg", _random_configs(72, 20261004), ids=lambda c: "N%d_d%d_g%d_a%d_e%d_p%d_o%d" % c)
def test_random_configurations_against_oracle(cfg):
    from bioem_amd.synthetic import Workload
    N, maxD, grid, algo, nEnv, nP, nO = cfg
    W = Workload(N=N, nP=nP, nOrient=nO, nEnv=nEnv, maxD=maxD, grid=grid, algo=algo, npts=150)
    try:
        sel = list(range(nP))
        want, const = oracle_on_workload(W, sel, nO, algo)
        _, got = run_workload(W, 0, nO)
        assert_workload_matches(got, want, const, sel)
    finally:
        W.engine.close()


def _write_mrc(path, data):
    import struct
    ns, nr, nc = data.shape
    hdr = np.zeros(256, dtype="<i4")
    hdr[0:4] = [nc, nr, ns, 2]
    hdr[7:10] = [nc, nr, ns]
    raw = hdr.tobytes()
    raw = raw[:40] + struct.pack("<6f", 100., 100., 100., 90., 90., 90.) + raw[64:]
    with open(path, "wb") as f:
        f.write(raw + data.astype("<f4").tobytes())


def test_config5_shape_mrc_input_256_write_prob_angles(tmp_path):
    """BASELINE config 5 shape at small counts: 256^2 particles read from MRC stacks (--ReadMRC --ReadMultipleMRC),
    WRITE_PROB_ANGLES on, through the drop-in CLI; oracle fed with the images exactly as the reader delivers them."""
    from bioem_amd import hostlib
    N, nP = 256, 4
    case, _ = setup_for("g2_n128")
    rng = np.random.default_rng(11)
    up = np.kron(case["maps"][:nP], np.ones((2, 2), dtype=np.float32))          # 128 -> 256
    stack = (3.0 * up + rng.normal(size=up.shape) + 7.0).astype(np.float32)     # un-normalised raw counts
    d = tmp_path
    _write_mrc(str(d / "a.mrc"), stack[:2])
    _write_mrc(str(d / "b.mrc"), stack[2:])
    with open(d / "list.txt", "w") as f:
        f.write(str(d / "a.mrc") + "\n" + str(d / "b.mrc") + "\n")
    iof.write_text_model(str(d / "model.txt"), case["model"])
    kw = [("PIXEL_SIZE", [1.0]), ("NUMBER_PIXELS", [N]), ("USE_QUATERNIONS", []), ("CTF_B_ENV", [2.0, 300.0, 2]),
          ("CTF_DEFOCUS", [1.0, 4.0, 2]), ("CTF_AMPLITUDE", [0.1, 0.1, 1]), ("DISPLACE_CENTER", [10, 1]),
          ("WRITE_PROB_ANGLES", [3])]
    iof.write_param_file(str(d / "param.txt"), kw)
    lines = case["orient_lines"][:9]
    with open(d / "orient.txt", "w") as f:
        f.write("%d\n" % len(lines) + "\n".join(lines) + "\n")
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    r = subprocess.run([exe, "--Modelfile", "model.txt", "--Particlesfile", "list.txt", "--Inputfile", "param.txt",
                        "--ReadOrientation", "orient.txt", "--ReadMRC", "--ReadMultipleMRC"], cwd=str(d),
                       env=dict(os.environ, BIOEM_GPUS="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    maps = hostlib.read_particles(str(d / "list.txt"), N, mode=2)
    assert maps.shape == (nP, N, N)
    S = orc.Setup(orc.parse_param_file(str(d / "param.txt")), case["model"], maps, lines)
    want, wang = S.run(1)
    mine = iof.parse_output_probabilities(open(d / "Output_Probabilities").read())
    ref = iof.parse_output_probabilities(orc.format_output_probabilities(S, want))
    for g, m in zip(ref, mine):
        assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
        assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])
    rows = orc.ang_prob_rows(S, want, wang)
    ma = iof.parse_ang_prob(str(d / "ANG_PROB"))
    for m_ in rows:
        assert len(ma[m_]) == 3
        for g, m in zip(rows[m_], ma[m_]):
            assert m["angles"] == [float("%.4f" % v) for v in S.angles[g["orient"]]]
            assert abs(g["logp"] - m["logp"]) <= 5e-3


def test_config3_shape_ten_ctfs_two_shards():
    """BASELINE config 3 shape at small counts: 224^2, 2 defocus x 5 envelope = 10 CTFs, two orientation shards
    with private probability blocks merged by the log-sum-exp rule, against the oracle's unsharded run."""
    import bioem_amd.engine as eng
    case, _ = setup_for("g7_n224")
    P = dict(case["P"])
    f32 = np.float32
    import math
    fac = math.pi * 2.0 * 10000 * float(P["elecwavel"])
    P["nPhase"], P["startPhase"], P["endPhase"] = 2, f32(1.0 * fac), f32(4.0 * fac)
    P["nEnv"], P["startEnv"], P["endEnv"] = 5, f32(2.0), f32(300.0)
    S = orc.Setup(P, case["model"], case["maps"], case["orient_lines"])
    assert S.nCTF == 10
    E = make_engine(S, 1)
    blocks = []
    for g in range(2):
        raw, _, _ = run_native(E, S, g * S.nAngles // 2, (g + 1) * S.nAngles // 2)
        blocks.append(raw.copy())
    merged = eng.merge_host(blocks, S.nMaps, S.nAngles, 0).view(eng.PROB_MAP_DTYPE)
    want, _ = S.run(1)
    assert_same_posterior(S, merged, want)
    E.close()


DIRECT_TOL = 2e-4  # relative, on the final log posterior: the sliding window adds 16 384 products in f32 per value


@pytest.mark.parametrize("name", ["g10_n64", "g9_n35_odd", "g2_n128", "g1_n48", "g18_n50"])
def test_direct_cross_correlation_against_oracle(name, monkeypatch):
    """BIOEM_CC_DIRECT=1 (BASELINE config 4): the cross-correlation as a sliding window in real space (k_c2r_* +
    k_compare_direct, no transform of the product) gives the oracle's posterior -- even, odd and 128^2 images,
    ALGO 1 and 2, particles uploaded as images."""
    case, S = setup_for(name)
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    for algo in case["algos"]:
        try:
            E = make_engine(S, algo, real_space_particles=True)
        except RuntimeError as e:
            if "BIOEM_CC_DIRECT" in str(e):
                pytest.skip("window or image beyond the direct kernel: " + str(e))
            raise
        assert E.kernel_signature.startswith("k_compare_direct")
        _, pmap, _ = run_native(E, S)
        want, _ = S.run(algo)
        for a, b in zip(pmap, want):
            la, lb = S.final_logp(a), S.final_logp(b)
            assert abs(la - lb) <= DIRECT_TOL * abs(lb), (la, lb)
            assert (a["orient"], a["conv"]) == (b["orient"], b["conv"])
        E.close()


def test_config4_direct_kernel_equals_the_transform_path(monkeypatch):
    """BASELINE config 4 at its own shape (128^2, +-10 px): both algorithms of the product on the same workload --
    per particle the same best orientation / CTF / displacement and the same log posterior within DIRECT_TOL."""
    from bioem_amd.synthetic import Workload
    kw = dict(N=128, nP=96, nOrient=192, nEnv=2, maxD=10)
    Wf = Workload(**kw)
    assert Wf.engine.kernel_signature.startswith("k_compare_fast")
    _, pf = run_workload(Wf, 0, Wf.nOrient)
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    Wd = Workload(**kw)
    assert Wd.engine.kernel_signature == "k_compare_direct<3, 8>"
    rawd, pdm = run_workload(Wd, 0, Wd.nOrient)
    rawd2, _ = run_workload(Wd, 0, Wd.nOrient)
    assert rawd.tobytes() == rawd2.tobytes()
    for f in ("orient", "conv", "cent_x", "cent_y"):
        assert np.array_equal(pf[f], pdm[f]), f
    lf = np.log(pf["Total"]) + pf["Constoadd"]
    ld = np.log(pdm["Total"]) + pdm["Constoadd"]
    assert np.abs(lf - ld).max() <= DIRECT_TOL * np.abs(lf).max()


def test_config4_shape_against_direct_real_space_correlation():
    """BASELINE config 4 (FFT-free sliding-window algorithm, 128^2, 4 608 orientations) has no implementation in the
    reference; what it would compute is the SAME posterior from the real-space cross-correlation
    cc(dx, dy) = sum_xy conv(x + dx, y + dy) * particle(x, y) (circular), the identity behind the c2r transform of
    bioem.cpp:1452-1458.  The product path at the config-4 shape is checked against that definition evaluated directly
    in float64 (numpy) with the oracle's calc_logpro, plus the size-independent properties."""
    import ctypes as C
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=128, nP=64, nOrient=4608, nEnv=1, maxD=10)
    N, mD = W.N, 10
    raw, full = run_workload(W, 0, W.nOrient)
    raw2, _ = run_workload(W, 0, W.nOrient)
    assert raw.tobytes() == raw2.tobytes()
    truth = (7919 * np.arange(W.nP)) % W.nOrient
    assert np.mean(full["orient"] == truth) > 0.9
    _, sumRef, sumsqRef = oracle_particle_inputs(W.maps, list(range(W.nP)))      # the oracle's own sums
    pd = orc.ParamDevice()
    for f, _ in orc.ParamDevice._fields_:
        setattr(pd, f, getattr(W.pd, f))
    amp, pha, env = (np.float32(v) for v in W.ctfParam[0])
    L = orc.lib()
    for p, o in [(0, int(truth[0])), (17, int(truth[17])), (63, 5)]:
        spec, sumC, sumsqC = W.engine.debug_convolution(o, 0)
        conv = np.fft.irfft2(spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64), s=(N, N))
        part = W.maps[p].astype(np.float64)
        lp = np.empty((2 * mD + 1, 2 * mD + 1))
        for dx in range(-mD, mD + 1):
            for dy in range(-mD, mD + 1):
                cc = np.float32(np.sum(np.roll(conv, (-dx, -dy), axis=(0, 1)) * part))
                lp[dx + mD, dy + mD] = L.orc_calc_logpro(C.byref(pd), amp, pha, env, sumC, sumsqC, cc, sumRef[p],
                                                         sumsqRef[p])
        m = lp.max()
        want = m + np.log(np.exp(lp - m).sum())
        bx, by = np.unravel_index(np.argmax(lp), lp.shape)
        r1, got = run_workload(W, o, o + 1)
        g = got[p]
        have = np.log(g["Total"]) + g["Constoadd"]
        assert abs(have - want) <= REL_TOL * abs(want) and abs(have - want) <= ABS_TOL
        # the reference reports the NEGATIVE displacement of the best match (bioem_algorithm.h:95-96)
        assert (g["orient"], g["conv"], g["cent_x"], g["cent_y"]) == (o, 0, -(bx - mD), -(by - mD))
    W.engine.close()


def test_cli_model_formats_pdb_and_mrc(tmp_path):
    """--ReadPDB and --ReadModelMRC through the CLI against the oracle fed with the same points."""
    from bioem_amd import hostlib
    case, _ = setup_for("g3_n32_trace")
    d = tmp_path
    iof.write_text_particles(str(d / "particles.txt"), case["maps"])
    with open(d / "orient.txt", "w") as f:
        f.write("%d\n" % len(case["orient_lines"]) + "\n".join(case["orient_lines"]) + "\n")
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    # PDB: C-alpha trace built from the golden model coordinates with cycling residue names
    names = ["GLY", "ALA", "TRP", "LYS", "GLU", "PHE"]
    with open(d / "m.pdb", "w") as f:
        for i, p in enumerate(case["model"]):
            f.write("ATOM  %5d  CA  %s A%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n"
                    % (i + 1, names[i % 6], i + 1, p[0], p[1], p[2]))
        f.write("END\n")
    # MRC density map: 6^3 voxels
    rng = np.random.default_rng(8)
    vol = rng.uniform(0.1, 1.0, size=(6, 6, 6)).astype(np.float32)
    hdr = np.zeros(256, dtype="<i4")
    hdr[0:4] = [6, 6, 6, 2]
    hdr[7:10] = [6, 6, 6]
    with open(d / "v.mrc", "wb") as f:
        f.write(hdr.tobytes() + vol.tobytes())
    for flag, mfile, kind in (("--ReadPDB", "m.pdb", dict(isPDB=True)), ("--ReadModelMRC", "v.mrc", dict(isMRC=True))):
        r = subprocess.run([exe, "--Modelfile", mfile, "--Particlesfile", "particles.txt", "--Inputfile",
                            os.path.join(case["dir"], "param.txt"), "--ReadOrientation", "orient.txt", flag,
                            "--OutputFile", "out_" + mfile], cwd=str(d), env=dict(os.environ, BIOEM_GPUS="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        pts, nd = hostlib.read_model(str(d / mfile), nocentermass=True, pixelSize=case["P"]["pixelSize"], **kind)
        arr = np.concatenate([pts["pos"].astype(np.float64), pts["radius"][:, None].astype(np.float64),
                              pts["density"][:, None].astype(np.float64)], axis=1)
        S = orc.Setup(case["P"], arr, case["maps"], case["orient_lines"])
        want, _ = S.run(1)
        ref = iof.parse_output_probabilities(orc.format_output_probabilities(S, want))
        mine = iof.parse_output_probabilities(open(d / ("out_" + mfile)).read())
        for g, m in zip(ref, mine):
            assert abs(g["logp"] - m["logp"]) <= max(ABS_TOL, REL_TOL * abs(g["logp"]))
            assert (g["angles"], g["ctf"], g["cx"], g["cy"]) == (m["angles"], m["ctf"], m["cx"], m["cy"])
