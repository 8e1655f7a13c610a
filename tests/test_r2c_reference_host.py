"""CPU tests of tests/r2c_reference.py: the reference against a full-mpmath transform, its two forms against each other,
seq_sums against the oracle, and the word rule against the reference's own rounding, against numpy's double transform
(which must pass) and against three mutants of the reference (which must fail) on the inputs of
tests/test_r2c_exact_gpu.py."""
import math

import numpy as np
import pytest

import r2c_reference as rr

LD = np.longdouble
f32 = np.float32

ALL_SIZES = sorted(set(rr.SIZES_A + rr.SIZES_B + rr.SIZES_B_DFT + rr.HANDLE_SIZES))


def m_max(N):
    """the most lenient m any GPU case applies at this size"""
    return max(rr.m_of(N), rr.m_of(N, True))


def rounded(re, im):
    return np.stack([re.astype(f32), im.astype(f32)], axis=-1)


@pytest.mark.parametrize("N", [4, 6, 9, 35])
def test_exact_r2c_against_mpmath(N):
    """every bin of a dense and a sparse image against the double sum in 200-bit arithmetic: 1e-18 sum|x|"""
    import mpmath
    H = N // 2 + 1
    with mpmath.workprec(200):
        def to_mp(v):
            d = float(v)
            return mpmath.mpf(d) + mpmath.mpf(float(v - LD(d)))
        w = [mpmath.expjpi(mpmath.mpf(-2 * t) / N) for t in range(N)]
        for j in (0, 1):
            img, _, _, sa = rr.case_image(N, j)
            re, im = rr.exact_r2c(img[None])
            nz = [(i, c, mpmath.mpf(float(img[i, c]))) for i in range(N) for c in range(N) if img[i, c] != 0]
            worst = mpmath.mpf(0)
            for u in range(N):
                for k in range(H):
                    ref = sum(a * w[(u * i + k * c) % N] for i, c, a in nz)
                    worst = max(worst, abs(to_mp(re[0, u, k]) - ref.real), abs(to_mp(im[0, u, k]) - ref.imag))
            assert worst <= mpmath.mpf("1e-18") * to_mp(sa), (N, j, worst)


@pytest.mark.parametrize("N", [4, 6, 9, 16, 23, 35, 64])
def test_exact_sparse_equals_exact_r2c(N):
    for j, t in ((0, False), (2, True)):
        px = rr.sparse_pixels(N, j)
        img = rr.image_of(N, px, transpose=t)
        assert np.count_nonzero(img) == N and (np.count_nonzero(img, axis=0) == 1).all()
        re, im = rr.exact_r2c(img[None])
        sre, sim = rr.exact_sparse(N, [(x, y, a) if t else (y, x, a) for y, x, a in px])
        tol = LD(1e-18) * LD(np.abs(img).sum())
        assert np.abs(re[0] - sre).max() <= tol and np.abs(im[0] - sim).max() <= tol


def test_inputs_are_what_they_claim():
    for N in (4, 16, 35, 289):
        px = rr.sparse_pixels(N, 0)
        assert sorted(p[0] for p in px) == sorted(p[1] for p in px) == list(range(N))
        a = np.array([p[2] for p in px])
        assert (a >= 0.5).all() and (a <= 2).all() and (a * 16 == np.rint(a * 16)).all()
        assert len(set(a[:25].tolist())) == min(N, 25)
        d = rr.dense_image(N, 1)
        assert (d == np.rint(d)).all() and d.min() >= -8 and d.max() <= 8
    img, _, _, _ = rr.case_image(16, 2)
    assert (img == rr.case_image(16, 2)[0]).all() and not img.flags.writeable


def test_m_stays_under_the_cap():
    """4 (A + B) + 32 for every size a GPU case uses and every split the fast transform compiles"""
    for N in ALL_SIZES + list(rr.HANDOVER) + [3080]:
        A, B = rr.split(N)
        for dft in (False, True):
            assert rr.m_of(N, dft) <= 4 * (A + B) + 32
    for A in range(2, 21):
        for B in range(A, 21):
            assert 9 <= rr.m("fft", A, B) <= 4 * (A + B) + 32
    assert rr.m("dft", 55, 56) == 3 * 56 + 4 * 55 + 8 and rr.m("mfma", 9, 23) == 3 * 24 + 4 * 12 + 8
    assert rr.m("fft", 16, 16) == 2 * (8 + 8) + 9


def test_kernel_selection_restated():
    fam = {N: (rr.family(N), rr.family(N, True)) for N in (4, 16, 256, 272, 289, 23, 46, 207, 153, 305, 3080, 400)}
    assert fam[4] == ("fft16", "mfma2") and fam[256] == ("fft16", "mfma2")
    assert fam[272][0] == "fft20" and fam[289] == ("fft20", "mfma5") and fam[400] == ("fft20", "dft_lds")
    assert fam[23][0] == "mfma2" and fam[46][0] == "mfma2" and fam[207][0] == "mfma5" and fam[153] == ("fft20", "mfma5")
    assert fam[305][0] == "dft_lds" and fam[3080][0] == "dft_global"
    assert all(rr.family(N, True) != "mfma5" for N in range(1, 153))          # 153 is the smallest
    assert rr.fft_plan(16) == (64, 4) and rr.fft_plan(20) == (51, 4) and rr.fft_plan(289) == (9, 3)


def check_caps(v, what):
    assert v.bad == 0, (what, str(v), v.first_bad)
    assert v.two <= 0.03 * v.words and v.subnormal <= 0.001 * v.words, (what, str(v))


@pytest.mark.parametrize("N", ALL_SIZES)
def test_rule_accepts_the_reference_and_numpy(N):
    """the reference's own rounding passes with share 0; numpy's double rfft2 passes; the loose words stay under the
    caps (two answers 3 %, subnormal 0.1 %) with the most lenient m of the size"""
    imgs, re, im, sa = rr.case_stack(N, 5 if N in (16, 35) else 3)
    for mm in {rr.m_of(N), m_max(N)}:
        v = rr.verdict(rounded(re, im), re, im, sa, mm)
        check_caps(v, N)
        assert v.share == 0.0
        v = rr.verdict(np.fft.rfft2(imgs.astype(np.float64)).astype(np.complex64), re, im, sa, mm)
        check_caps(v, ("numpy", N))
    for b in range(len(imgs)):                              # the caps hold per image, not only per stack
        check_caps(rr.verdict(rounded(re[b], im[b]), re[b], im[b], sa[b], m_max(N)), (N, b))


@pytest.mark.parametrize("N", sorted(rr.HANDOVER))
def test_rule_accepts_the_handover_images(N):
    dft, distinct = rr.HANDOVER[N]
    imgs, re, im, sa = rr.case_stack(N, distinct)
    check_caps(rr.verdict(rounded(re, im), re, im, sa, rr.m_of(N, dft)), N)


def test_rule_accepts_the_big_sparse_image():
    N, px = 3080, rr.big_sparse()
    assert len({p[0] for p in px}) == len({p[1] for p in px}) == 8
    assert len({p[0] % 55 for p in px}) > 4 and len({p[1] % 56 for p in px}) > 4
    re, im = rr.exact_sparse(N, px)
    check_caps(rr.verdict(rounded(re, im), re, im, sum(f32(p[2]) for p in px), rr.m_of(N)), N)


def series_cis(N, terms):
    """cos and sin of 2 pi k / N by octant reduction and a Taylor series of `terms` terms in double"""
    c, s = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)
    for k in range(N):
        n, T = 8 * k, 8 * N
        neg_s = neg_c = swap = False
        if n > T // 2:
            n, neg_s = T - n, True
        if n > T // 4:
            n, neg_c = T // 2 - n, True
        if n > T // 8:
            n, swap = T // 4 - n, True
        x = 2.0 * math.pi * n / T
        cc, ss, tc, ts = 1.0, x, 1.0, x
        for j in range(1, terms):
            tc *= -x * x / ((2 * j - 1) * (2 * j))
            ts *= -x * x / ((2 * j) * (2 * j + 1))
            cc += tc
            ss += ts
        if n == 0:
            cc, ss = 1.0, 0.0
        if swap:
            cc, ss = ss, cc
        c[k], s[k] = (-cc if neg_c else cc), (-ss if neg_s else ss)
    return c, s


@pytest.mark.parametrize("N", ALL_SIZES)
def test_mutants_of_the_reference_fail(N):
    """the row pass rounded to float32, a cis table rounded to float32, a cis series of 6 terms.  A mutant can only be
    seen where it moves a value over a float midpoint.  At N = 4 the table is 0, +-1 and every intermediate an exact
    float: the three are the reference.  The float32 mutants are off by 2^-25 of a term, a quarter of the way to a
    midpoint: they must fail from N = 6 on.  The series is off by at most (pi / 4)^12 / 12! = 1.2e-10, 2e-3 of the way:
    it needs a thousand words, so it must fail from N = 20 on (3 * 20 * 11 * 2 words); below that its count is printed.
    A series of 14 terms, the product's, passes.  Above 100 pixels the dense image alone (time)."""
    if N <= 100:
        imgs, re, im, sa = rr.case_stack(N, 3)
    else:
        imgs, re, im, sa = (a[1:2] for a in rr.case_stack(N, 2))
    c, cl, s, sl = rr.cis_table(N)
    mutants = {
        "rows32": lambda: rr._two_pass(imgs, c, s, cl, sl, round_rows=f32),
        "cis32": lambda: rr._two_pass(imgs, c.astype(f32).astype(LD), s.astype(f32).astype(LD)),
        "series6": lambda: rr._two_pass(imgs, *series_cis(N, 6)),
    }
    for name, run in mutants.items():
        v = rr.verdict(rounded(*run()), re, im, sa, m_max(N))
        print("N %d %s: %s" % (N, name, v))
        if N == 4:
            assert v.bad == 0
        elif name != "series6" or N >= 20:
            assert v.bad > 0, (N, name)
    if N <= 100:
        v = rr.verdict(rounded(*rr._two_pass(imgs, *series_cis(N, 14))), re, im, sa, rr.m_of(N))
        assert v.bad == 0, str(v)


def test_verdict_classes_by_hand():
    """one word of each class, and each way to fail"""
    E = LD(8) * rr.U53 * LD(4.0)                             # m = 8, sum|x| = 4
    one, up = f32(1.0), np.nextafter(f32(1.0), f32(2.0))
    mid = (LD(one) + LD(up)) / 2

    def run(got, exact):
        return rr.verdict(np.array([[got, 0.0]], dtype=f32), np.array([exact], dtype=LD), np.array([0], dtype=LD), 4.0, 8)
    v = run(one, LD(1) + 3 * E)
    assert (v.one, v.two, v.small, v.bad) == (1, 0, 1, 0)
    assert run(up, LD(1) + 3 * E).bad == 1                   # one answer: the neighbour fails
    v = run(up, mid - E / 2)                                 # two answers: either passes, the far one proves E / 2
    assert (v.two, v.bad) == (1, 0) and abs(v.share - 0.5) < 1e-6
    v = run(one, mid - E / 2)
    assert (v.two, v.bad, v.share) == (1, 0, 0.0)
    assert run(np.nextafter(up, f32(2.0)), mid - E / 2).bad == 1
    assert run(one, mid + 2 * E).bad == 1 and run(up, mid + 2 * E).bad == 0
    v = run(f32(E / 2), LD(0))                               # small
    assert (v.small, v.bad) == (2, 0) and abs(v.share - 0.5) < 1e-6
    assert run(f32(3 * E), LD(0)).bad == 1
    assert run(f32("nan"), LD(1)).bad == 1 and run(f32("nan"), LD(0)).bad == 1
    sub = rr.verdict(np.array([[0.0, 0.0]], dtype=f32), np.array([LD(2.0) ** -130]), np.array([0], dtype=LD), 1e-30, 8)
    assert (sub.subnormal, sub.bad) == (1, 0)


def test_seq_sums_is_sequential_and_equals_the_oracle():
    import oracle as orc
    for N in (5, 63, 64, 65, 91):
        for b in range(3):
            img = rr.wide_image(N, b)
            s = s2 = f32(0)
            for v in img.reshape(-1):
                s = f32(s + v)
                s2 = f32(s2 + f32(v * v))
            got = rr.seq_sums(img)
            assert (got[0], got[1]) == (s, s2)
            o = orc.map_sums(img)
            assert (f32(o[0]).tobytes(), f32(o[1]).tobytes()) == (got[0].tobytes(), got[1].tobytes())
