"""GPU tests of the r2c kernels (k_r2c_fft<*, 16 | 20, 3>, k_dft_rows_mfma / k_dft_cols_mfma<2 | 5>, k_dft_rows /
k_dft_cols<true | false>) and of k_map_sums, word by word against the exact reference of tests/r2c_reference.py
(DESIGN 2.25).  Through bioem_amd.engine.r2c unless stated.

Every float word must be the float nearest a value within E = m 2^-53 sum|x| of the exact one (classes one answer / two
answers / small / subnormal, r2c_reference.verdict); each case prints its counts and the largest share of E its loose
words prove.  m is derived in r2c_reference.m from the kernel sources and was fixed before the first run.

Which case reaches which instantiation (r2c_reference.family restates the launchers; the cases assert it):
  k_r2c_fft<true | false, 16, 3>      (a) every N with B <= 16: 4 ... 256; (d) 16, 20; (e) 35, 64, 256
  k_r2c_fft<true | false, 20, 3>      (a) 272, 289, 324, 361, 380, 400; (d) 289
  k_dft_rows_mfma<2>, k_dft_cols_mfma<2>   (a) BIOEM_R2C=dft, N <= 100; (b) 23, 46; (d) 23
  k_dft_rows_mfma<5>, k_dft_cols_mfma<5>   (a) BIOEM_R2C=dft, 289; (b) 207 by default, 153 under BIOEM_R2C=dft; (d) 153
  k_dft_rows<true>, k_dft_cols<true>       (b) 305
  k_dft_rows<false>, k_dft_cols<false>     (b) 3080, one image of 8 pixels against the closed form

Largest share of E per case, measured on an MI355X (0.000 where no loose word of the case crossed its midpoint; the
loose words are few -- at most 0.07 % of a case are two answers -- so the shares say "no slip seen", not "this much used"):
  (a) default path   0.022 at 6, 0.001 at 380, 0.000 at the 22 other sizes; ragged stacks 0.000
  (a) BIOEM_R2C=dft  0.021 at 4, 0.101 at 6, 0.017 at 16, 0.014 at 20, 0.009 at 36 and 64, 0.006 at 100, else 0.000
  (b) 23: 0.000   46: 0.006   207: 0.000   153 (dft): 0.000   305: 0.000   3080: 0.008 (1.9 s, one image)
  (c) the two paths differ in 0 to 12 words per size, all of them small words (the exact zeros of self-conjugate bins)
  (d) 16 (24 877 images), 20 (15 881), 23 (3 098), 153 (154), 289 (144) on 256 CUs: 0.000, all copies bit-equal
  (e) 35, 64, 256: 0.000          (f) bit for bit
  tests/test_projection_exact_gpu.py, double input and boxes: 0.010 at most (64 under BIOEM_R2C=dft), 0.007 at 46

Strength: one scratch copy of the library per slip, none committed.  "old" = test_fast_r2c_against_numpy_and_the_exact_dft
and the r2c tests of tests/test_projection_exact_gpu.py as they were (40 tests); "new" = this file and that one now (86).
  stage-1 twiddle product of r2c_stage1 in float   old 32 fail, all by the 2 % allowance between the two paths (the
                                                   1.5e-7 bound passes); new 55 fail: every fast-path case from 6 on
  r2c_cis with 6 series terms                      old 0 of 40 fail; new 44 fail: every fast-path size but 4, 9, 16 and 36,
                                                   whose butterflies use no series entry that the cut moves by a midpoint
  twiddle_d rounded through float                  old 31 fail, again by the 2 % allowance only; new 77 fail (all families,
                                                   3080 included; 4 passes: its table is 0 and +-1)
  v0 / v1 swapped for the self-paired last row     old 0, new 0: an equivalent slip -- both reads are the same word
  sign of the second separated row flipped         old 37 fail; new 57 fail
  Gp = G for G | 1                                 old 0, new 0, as it must: the results are pinned, not the layout
"""
import numpy as np
import pytest

import r2c_reference as rr

pytestmark = pytest.mark.gpu

f32 = np.float32
_GOT = {}


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def device_r2c(images, dft, monkeypatch):
    from bioem_amd import engine as eng
    if dft:
        monkeypatch.setenv("BIOEM_R2C", "dft")
    else:
        monkeypatch.delenv("BIOEM_R2C", raising=False)
    return eng.r2c(images)


def spectrum(N, dft, monkeypatch):
    """the device's transform of the three case images of N, computed once per path"""
    if (N, dft) not in _GOT:
        _GOT[N, dft] = device_r2c(rr.case_stack(N)[0], dft, monkeypatch)
    return _GOT[N, dft]


def judge(what, got, re, im, sa, m):
    v = rr.verdict(got, re, im, sa, m)
    print("%s: m %d  %s" % (what, m, v))
    assert v.bad == 0, (what, v.first_bad)
    assert v.share <= 1.0
    return v


# ---- (a) every sub-transform length ----
@pytest.mark.parametrize("N,dft", [(N, False) for N in rr.SIZES_A] + [(N, True) for N in rr.SIZES_A_DFT])
def test_every_length_bin_by_bin(N, dft, monkeypatch):
    """N = L^2, L = 2 ... 20: every compiled length in both stages; 6, 20, 35, 380; the LMAX boundary 256, 272, 289.
    sparse, dense, sparse transposed.  BIOEM_R2C=dft: the matrix-core kernels, <2> up to 100 and <5> at 289"""
    A, B = rr.split(N)
    want = ("mfma5" if N == 289 else "mfma2") if dft else ("fft16" if B <= 16 else "fft20")
    assert rr.family(N, dft) == want
    _, re, im, sa = rr.case_stack(N)
    judge("N %d (%d x %d) %s" % (N, A, B, want), spectrum(N, dft, monkeypatch), re, im, sa, rr.m_of(N, dft))


@pytest.mark.parametrize("N,n", rr.RAGGED)
def test_ragged_last_units(N, n, monkeypatch):
    """1, 2 and 5 images: the last unit of the row and of the column launch ends inside a group (but 2 images of 35
    pixels, which fill their one unit of 36 transforms exactly)"""
    imgs, re, im, sa = rr.case_stack(N, n)
    G, _ = rr.fft_plan(N)
    tails = [((k * ((N + 1) // 2)) % G, (k * (N // 2 + 1)) % G) for k in (1, 2, 5)]
    assert sum(r != 0 and c != 0 for r, c in tails) >= 2, tails
    judge("N %d, %d images" % (N, n), device_r2c(imgs, False, monkeypatch), re, im, sa, rr.m_of(N))


# ---- (b) the sizes that take the exact-DFT kernels in production ----
@pytest.mark.parametrize("N,dft,want", [(23, False, "mfma2"), (46, False, "mfma2"), (207, False, "mfma5"),
                                        (153, True, "mfma5"), (305, False, "dft_lds")])
def test_exact_dft_sizes(N, dft, want, monkeypatch):
    assert rr.family(N, dft) == want
    _, re, im, sa = rr.case_stack(N)
    judge("N %d (%d x %d) %s" % ((N,) + rr.split(N) + (want,)), spectrum(N, dft, monkeypatch), re, im, sa, rr.m_of(N, dft))


def test_twiddles_from_global_memory_at_3080():
    """k_dft_rows<false> / k_dft_cols<false> (55 x 56, beyond the 3072 pixels whose table fits LDS): one image of 8
    pixels against the closed form"""
    from bioem_amd import engine as eng
    N, px = 3080, rr.big_sparse()
    assert rr.family(N) == "dft_global" and rr.split(N) == (55, 56)
    got = eng.r2c(rr.image_of(N, px)[None])
    re, im = rr.exact_sparse(N, px)
    judge("N 3080 dft_global", got[0], re, im, sum(f32(p[2]) for p in px), rr.m_of(N))


# ---- (c) the fast transform against the exact DFT ----
@pytest.mark.parametrize("N", rr.SIZES_A_DFT + rr.SIZES_B_DFT)
def test_fast_equals_exact_dft_but_for_loose_words(N, monkeypatch):
    """the two paths give the same word wherever the rule allows one answer (under the larger m of the two)"""
    assert rr.family(N).startswith("fft") and rr.family(N, True).startswith("mfma")
    _, re, im, sa = rr.case_stack(N)
    fast, slow = rr.words_of(spectrum(N, False, monkeypatch)), rr.words_of(spectrum(N, True, monkeypatch))
    v = judge("N %d exact DFT" % N, slow, re, im, sa, max(rr.m_of(N, True), rr.m_of(N)))
    differ = fast.view(np.uint32) != slow.view(np.uint32)
    signed_zero = (fast == 0) & (slow == 0)
    print("N %d: %d of %d words differ, %d loose" % (N, differ.sum(), differ.size, v.loose.sum()))
    assert not (differ & ~v.loose & ~signed_zero).any(), np.argwhere(differ & ~v.loose)[:5]


# ---- (d) the hand-over from unit to unit ----
def images_for_three_units(N, dft, n_cu):
    n = 1
    while any(u < 3 * g for u, g in rr.units_and_grid(N, n, n_cu, dft)):
        n += max(1, n // 64)
    return n


@pytest.mark.parametrize("N", sorted(rr.HANDOVER))
def test_unit_handover(N, monkeypatch):
    """every block of the resident grid walks at least three units, so the LDS area is handed from unit to unit behind
    the loop's barrier; a shuffled stack of a few distinct images: every copy passes, copies agree bit for bit"""
    dft, distinct = rr.HANDOVER[N]
    n_cu = compute_units()
    n = images_for_three_units(N, dft, n_cu)
    fam = rr.family(N, dft)
    assert fam == {16: "fft16", 20: "fft16", 289: "fft20", 23: "mfma2", 153: "mfma5"}[N]
    # the planner's arithmetic, restated: G transforms per unit and at most 4 blocks per CU (fast), 16 rows / columns per
    # unit and at most 4 (<2>) or 1 (<5>) blocks per CU (matrix cores)
    H = N // 2 + 1
    if fam.startswith("fft"):
        G, per_cu = rr.fft_plan(N)
        assert (G, per_cu) == {16: (64, 4), 20: (51, 4), 289: (9, 3)}[N]
        units = [-(-n * ((N + 1) // 2) // G), -(-n * H // G)]
    else:
        per_cu = 4 if fam == "mfma2" else 1
        units = [n * ((N + 15) // 16), n * ((H + 15) // 16)]
    assert min(units) >= 3 * per_cu * n_cu, (units, per_cu, n_cu)
    imgs, re, im, sa = rr.case_stack(N, distinct)
    order = np.random.default_rng(N).permutation(np.arange(n) % distinct)
    got = device_r2c(imgs[order], dft, monkeypatch)
    print("N %d %s: %d images, units %s, grid %d" % (N, fam, n, units, per_cu * n_cu))
    first = np.array([np.nonzero(order == j)[0][0] for j in range(distinct)])
    judge("N %d hand-over, the first copies" % N, got[first], re, im, sa, rr.m_of(N, dft))
    same = got.view(np.uint32) == got[first][order].view(np.uint32)
    assert same.all(), np.argwhere(~same)[:5]


# ---- (e) through a handle ----
def make_engine(N, n_maps):
    import bioem_amd.engine as eng
    pd = eng.ParamDevice()
    pd.maxDisplaceCenter, pd.GridSpaceCenter, pd.NumberPixels, pd.NumberFFTPixels1D = 2, 1, N, N // 2 + 1
    pd.NxDisp, pd.NtotDisp, pd.Ntotpi, pd.volu = 5, 25, float(N * N), 1.0
    pd.sigmaPriorbctf, pd.sigmaPriordefo, pd.Priordefcent, pd.sigmaPrioramp, pd.Priorampcent = 100.0, 2.0, 3.0, 0.5, 0.0
    return eng.Engine(pd, n_maps, 4, 1, algo=1, device=0)


@pytest.mark.parametrize("N", rr.HANDLE_SIZES)
def test_particles_through_a_handle(N, monkeypatch):
    """upload_particle_maps transforms in chunks of max(32, max_batch()[0]) images into the comparison layout (generic
    at 35, fast at 64, fast with a padded pitch at 256); one particle more than two chunks.  What debug_particles reads
    back is r2c() of the same images to the bit, and upload_particles returns its input to the bit"""
    monkeypatch.delenv("BIOEM_R2C", raising=False)
    from bioem_amd import engine as eng
    n_maps = 65
    E = make_engine(N, n_maps)
    try:
        chunk = max(32, E.max_batch()[0])
        assert n_maps % chunk == 1 and n_maps > chunk
        print("N %d: %s, fast path %d" % (N, E.kernel_name if hasattr(E, "kernel_name") else "", E.fast_path))
        imgs, re, im, sa = rr.case_stack(N, 3)
        order = np.arange(n_maps) % 3
        stack = np.ascontiguousarray(imgs[order])
        E.upload_particle_maps(stack)
        spec, s, s2 = E.debug_particles()
        direct = eng.r2c(stack)
        assert spec.tobytes() == rr.words_of(direct).tobytes()
        judge("N %d through a handle" % N, spec, re[order], im[order], sa[order], rr.m_of(N))
        sums = [rr.seq_sums(m) for m in imgs]
        assert s.tobytes() == np.array([sums[j][0] for j in order], dtype=f32).tobytes()
        assert s2.tobytes() == np.array([sums[j][1] for j in order], dtype=f32).tobytes()
        rng = np.random.default_rng(N)
        given = rng.standard_normal(spec.shape).astype(f32)
        given[0, 0, 0] = [-0.0, np.float32(1e-40)]           # a signed zero and a subnormal travel unchanged
        gs, gs2 = rng.standard_normal(n_maps).astype(f32), rng.standard_normal(n_maps).astype(f32)
        E.upload_particles(given, gs, gs2)
        back, bs, bs2 = E.debug_particles()
        assert back.tobytes() == given.tobytes() and bs.tobytes() == gs.tobytes() and bs2.tobytes() == gs2.tobytes()
    finally:
        E.close()


# ---- (f) k_map_sums ----
@pytest.mark.parametrize("N", rr.SUM_SIZES)
def test_map_sums_at_the_chunk_edges(N):
    """k_map_sums folds 4096-float chunks through LDS: N^2 = 4096 - 127, 4096, 4096 + 129, 2 * 4096 + 89, 4 * 4096.
    Sum and sum of squares of three wide-range images equal the sequential float32 sums bit for bit"""
    assert N * N == {63: 4096 - 127, 64: 4096, 65: 4096 + 129, 91: 2 * 4096 + 89, 128: 4 * 4096}[N]
    maps = np.stack([rr.wide_image(N, b) for b in range(3)])
    E = make_engine(N, 3)
    try:
        E.upload_particle_maps(maps)
        _, s, s2 = E.debug_particles()
    finally:
        E.close()
    want = [rr.seq_sums(m) for m in maps]
    assert s.tobytes() == np.array([w[0] for w in want], dtype=f32).tobytes(), (s, want)
    assert s2.tobytes() == np.array([w[1] for w in want], dtype=f32).tobytes(), (s2, want)
