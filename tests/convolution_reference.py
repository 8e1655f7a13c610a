"""Reference of the convolution stage (reference bioem.cpp:1855-1923; the kernels k_convolve + k_parseval_ordered and
k_convolve_sums): conv = proj conj(CTF), sumC = Re conv[0][0], sumsquareC = the sequential float sum of |conv|^2 in the
reference's order, divided by N^2.  Shares no code with the product and does not call the library.

    conv_exact(proj, ctf)          the product in float64 (every product of two floats is exact there) and the per-bin
                                   magnitudes |p.x k.x| + |p.y k.y|, |p.y k.x| + |p.x k.y| that bound its rounding
    conv_f32(proj, ctf)            the reference's expression, one float32 rounding per written operation
    parseval_order(N)              bins and weights 2/1/1 in the order bioem.cpp:1896-1914 adds them
    chain_f32(terms)               the sequential float32 sum along the last axis
    sumsquare_ordered(conv, N)     f32(chain / f32(N N)) over the ordered terms of a float32 spectrum
    comparison_layout(spec, fast, N1, Hp)   the comparison kernels' layout of a spectrum, stated on its own
    class_a(N), class_b(N)         the two input classes of tests/test_convolution_exact_gpu.py

Class A is exact whatever a compiler fuses: every component is a small integer (or a power of two times one), so every
product, every sum of two products and every Parseval term is representable -- an FMA and a multiply-add round the same,
namely not at all -- and only the additions of the chain round.  Planted bins that weigh 2^25 lift the running sum to
where an addition of a small term rounds, so the value of the chain depends on the order of its terms."""
import numpy as np

f32, f64 = np.float32, np.float64

N_ORIENT, N_CTF = 7, 13                      # what the largest launch shape of the GPU test takes
SIZES = [9, 10, 21, 35, 44, 64, 75, 96, 192]
# (nO, c0, nC): k_convolve_sums<4, 4> with blocks 4 + 1 and 4 + 3; <3, 5> with 3 + 1 and 3 + 3 + 1; <3, 6> with CTF groups
# 6, 6 + 1 and 6 + 6 + 1; nO nC = 1, 15, 28, 20, 5, 20, 35, 12, 28, 91, 21, 5 rows for k_parseval_ordered (every residue mod 4)
SHAPES = [(1, 0, 1), (5, 0, 3), (7, 0, 4), (5, 9, 4),
          (1, 0, 5), (4, 0, 5), (7, 8, 5),
          (2, 0, 6), (4, 0, 7), (7, 0, 13), (3, 6, 7), (5, 12, 1)]
SHAPES_192 = [(4, 0, 7), (2, 8, 5)]
TILE_FUSED, TILE_ORDERED = 960, 512          # terms per tile of k_convolve_sums and of k_parseval_ordered
# the seed of each size's class-A set: the first from 1 on whose set meets the conditions of
# tests/test_convolution_reference_host.py (distinct sums, every launch shape sensitive to each of the five wrong orders)
CLASS_A_SEED = {8: 5, 9: 17, 10: 5, 21: 1, 35: 1, 44: 1, 64: 2, 75: 3, 96: 4, 192: 2}
BASE_PLACE = 1                               # the second term of the chain: 2^25 in every slot of class A
PRIMES = [11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59]


def shapes_of(N):
    return SHAPES_192 if N == 192 else SHAPES


def conv_exact(proj, ctf):
    """proj [..., 2], ctf [..., 2] float32 (broadcast against each other): (re, im, mag_re, mag_im) float64.  The four
    products are exact in double; re and im are one double addition away from exact (2^-53 of the magnitude)"""
    assert proj.dtype == f32 and ctf.dtype == f32
    px, py, kx, ky = (a.astype(f64) for a in (proj[..., 0], proj[..., 1], ctf[..., 0], ctf[..., 1]))
    a, b, c, d = px * kx, py * ky, py * kx, px * ky
    return a + b, c - d, np.abs(a) + np.abs(b), np.abs(c) + np.abs(d)


def conv_f32(proj, ctf):
    """bioem.cpp:1879-1882 in float32, nothing fused: [..., 2]"""
    assert proj.dtype == f32 and ctf.dtype == f32
    px, py, kx, ky = proj[..., 0], proj[..., 1], ctf[..., 0], ctf[..., 1]
    out = np.stack([px * kx + py * ky, py * kx - px * ky], axis=-1)
    assert out.dtype == f32
    return out


def parseval_order(N):
    """(bins, weights): bins[t] = i H + j of the t-th term the reference adds, weights[t] its factor.  Per row i: the
    columns 1 <= j < jloopend doubled, then column 0, then -- even N -- column N / 2 (bioem.cpp:1893-1914)"""
    H = N // 2 + 1
    jloopend = H - 1 if N % 2 == 0 else H
    bins, weights = [], []
    for i in range(N):
        for j in range(1, jloopend):
            bins.append(i * H + j)
            weights.append(2)
        bins.append(i * H)
        weights.append(1)
        if N % 2 == 0:
            bins.append(i * H + H - 1)
            weights.append(1)
    assert sorted(bins) == list(range(N * H))
    return np.array(bins), np.array(weights, dtype=f32)


def ordered_terms(conv, N):
    """conv float32 [..., N, H, 2]: the terms (x x + y y) (* 2) in float32, in the reference's order: [..., M]"""
    assert conv.dtype == f32
    bins, weights = parseval_order(N)
    x, y = conv[..., 0], conv[..., 1]
    t = (x * x + y * y).reshape(conv.shape[:-3] + (-1,))
    out = t[..., bins] * weights
    assert out.dtype == f32
    return out


def chain_f32(terms):
    """the sequential float32 sum along the last axis, from 0: one rounding per addition"""
    terms = np.asarray(terms)
    assert terms.dtype == f32
    s = np.zeros(terms.shape[:-1], dtype=f32)
    for t in range(terms.shape[-1]):
        s = s + terms[..., t]
    assert s.dtype == f32
    return s


def divide_f32(ss, N):
    return (np.asarray(ss, dtype=f32) / f32(N * N)).astype(f32)


def sumsquare_ordered(conv, N):
    return divide_f32(chain_f32(ordered_terms(conv, N)), N)


def comparison_layout(spec, fast, N1, Hp):
    """spec [N, H, 2] -> (raw [N Hp, 2] float32, data [N Hp] bool).  fast = 0: the reference layout, Hp = H.  Otherwise
    N = N1 * 2 fast and 16-byte word rp Hp + j, rp = k1 fast + k2p, holds column j of the rows i0 = N1 2 k2p + k1 (first
    8 bytes) and i0 + N1 (last 8); data marks the float2 that hold a bin (columns [H, Hp) of a row pair are padding)"""
    N, H = spec.shape[:2]
    if not fast:
        assert Hp == H
        return np.ascontiguousarray(spec, dtype=f32).reshape(N * H, 2).copy(), np.ones(N * H, dtype=bool)
    assert N == N1 * 2 * fast and Hp >= H
    words = np.zeros((N // 2, Hp, 2, 2), dtype=f32)
    data = np.zeros((N // 2, Hp, 2), dtype=bool)
    for k1 in range(N1):
        for k2p in range(fast):
            rp, i0 = k1 * fast + k2p, N1 * 2 * k2p + k1
            words[rp, :H, 0] = spec[i0]
            words[rp, :H, 1] = spec[i0 + N1]
            data[rp, :H] = True
    return words.reshape(N * Hp, 2), data.reshape(N * Hp)


def from_comparison_layout(raw, N, fast, N1, Hp):
    """the inverse of comparison_layout, written the other way round: per row kx where its bins lie"""
    H = N // 2 + 1
    if not fast:
        return raw.reshape(N, H, 2).copy()
    raw = raw.reshape(N // 2, Hp, 2, 2)
    spec = np.zeros((N, H, 2), dtype=f32)
    for kx in range(N):
        k1, k2 = kx % N1, kx // N1
        spec[kx] = raw[k1 * fast + k2 // 2, :H, k2 % 2]
    return spec


# ---- input class A: integer spectra with planted bins ----
def planted_positions(N, rng):
    """N_ORIENT + N_CTF distinct places in the summation order, the origin not among them: the first and the last term,
    column 0 and the Nyquist column of a row, the last term of a tile and the first of the next for tiles of 960 and of
    512 terms, a place inside the last partial float4 (the last three terms where M % 4 = 0), then random ones"""
    H = N // 2 + 1
    M = N * H
    bins, weights = parseval_order(N)
    origin = int(np.nonzero(bins == 0)[0][0])
    row = N // 2
    want = [0, M - 1, int(np.nonzero(bins == row * H)[0][0])]
    if N % 2 == 0:
        want.append(int(np.nonzero(bins == row * H + H - 1)[0][0]))
    for tile in (TILE_FUSED, TILE_ORDERED):
        for k in range(1, 3):
            want += [k * tile - 1, k * tile]
    want += [M - 2 if M % 4 != 1 else M - 1, (M & ~3) - 1, M & ~3]
    out = []
    for p in want:
        if 0 <= p < M and p not in (origin, BASE_PLACE) and p not in out:
            out.append(p)
    free = [p for p in rng.permutation(M).tolist() if p not in (origin, BASE_PLACE) and p not in out]
    out = (out + free)[:N_ORIENT + N_CTF]
    assert len(set(out)) == N_ORIENT + N_CTF
    return out, bins


class ClassA:
    """proj [N_ORIENT, N, H, 2] with components in [-3, 3], ctf [N_CTF, N, H, 2] in [-2, 2], all integers.  Orientation
    o has the planted bin b_o: proj_o = (2048, 0) there and every CTF (2, 0) -- (2, -2) where the term is not doubled --;
    CTF c has d_c: ctf_c = (2048, 0) or (2048, -2048) there and every orientation (2, 0).  A planted bin weighs 2^25 in
    the chain (4096^2 doubled, or 4096^2 + 4096^2).  A slot (o, c) holds exactly three: its orientation's and its CTF's,
    a pair of places no other slot has, and the base bin every slot has at the second place of the order (proj = (2048,
    0), ctf = (2, 0)): from there on the sum rounds to multiples of 4, then 8, against terms of 64 on average, and stays
    below 2^27.  (One bin of 2^26 per slot cannot sit at a place of the orientation's own and of the CTF's own at once;
    two halves can.  Without the base bin a slot whose planted bins come late adds exactly for most of its chain.)
    The origin holds proj_o = (o + 1, 1), ctf_c = (p_c, 1) with p_c the c-th prime from 11: sumC = (o + 1) p_c + 1,
    pairwise distinct.  conv, sumC, sumsq: the float32 expressions and chain of this module (equal to the oracle's bit
    for bit, tests/test_convolution_reference_host.py)"""

    def __init__(self, N, seed=None):
        seed = CLASS_A_SEED[N] if seed is None else seed
        rng = np.random.default_rng([N, seed])
        H = N // 2 + 1
        self.N, self.H, self.M, self.seed = N, H, N * H, seed
        proj = rng.integers(-3, 4, (N_ORIENT, N * H, 2)).astype(f32)
        ctf = rng.integers(-2, 3, (N_CTF, N * H, 2)).astype(f32)
        self.places, bins = planted_positions(N, rng)
        # alternately a CTF's and an orientation's, so that the first slots of a batch see the special places
        self.place_ctf = [self.places[2 * k] if k < N_ORIENT else self.places[N_ORIENT + k] for k in range(N_CTF)]
        self.place_orient = [self.places[2 * k + 1] for k in range(N_ORIENT)]
        assert sorted(self.place_ctf + self.place_orient) == sorted(self.places)
        weights = parseval_order(N)[1]
        assert weights[BASE_PLACE] == 2
        proj[:, bins[BASE_PLACE]] = (2048, 0)
        ctf[:, bins[BASE_PLACE]] = (2, 0)
        for o, p in enumerate(self.place_orient):
            ctf[:, bins[p]] = (2, 0) if weights[p] == 2 else (2, -2)
            proj[o, bins[p]] = (2048, 0)
        for c, p in enumerate(self.place_ctf):
            proj[:, bins[p]] = (2, 0)
            ctf[c, bins[p]] = (2048, 0) if weights[p] == 2 else (2048, -2048)
        proj[:, 0] = [(o + 1, 1) for o in range(N_ORIENT)]
        ctf[:, 0] = [(p, 1) for p in PRIMES]
        self.proj = proj.reshape(N_ORIENT, N, H, 2)
        self.ctf = ctf.reshape(N_CTF, N, H, 2)
        self.ctf_param = np.array([[0.0625 * (c + 1), 1.5 - 0.125 * c, 100.0 + 3 * c] for c in range(N_CTF)], dtype=f32)
        assert len({tuple(r) for r in self.ctf_param.tolist()}) == N_CTF
        self.conv = conv_f32(self.proj[:, None], self.ctf[None])                 # [o, c, N, H, 2]
        re, im, _, _ = conv_exact(self.proj[:, None], self.ctf[None])
        assert (self.conv[..., 0] == re).all() and (self.conv[..., 1] == im).all()  # no product rounded
        self.terms = ordered_terms(self.conv, N)                                 # [o, c, M]
        x, y = self.conv[..., 0].astype(f64), self.conv[..., 1].astype(f64)
        exact = (x * x + y * y).reshape(N_ORIENT, N_CTF, -1)[..., bins] * parseval_order(N)[1]
        assert (self.terms == exact).all()                                       # no term rounded
        assert ((self.terms == 2.0 ** 25).sum(axis=-1) == 3).all() and self.terms.max() == 2.0 ** 25
        self.sumC = self.conv[:, :, 0, 0, 0].copy()
        self.chain = chain_f32(self.terms)
        self.sumsq = divide_f32(self.chain, N)

    def distinct(self):
        """all sumC pairwise distinct, all sumsquareC pairwise distinct"""
        n = N_ORIENT * N_CTF
        return len(set(self.sumC.reshape(-1).tolist())) == n and len(set(self.sumsq.reshape(-1).tolist())) == n


_class_a = {}


def class_a(N):
    if N not in _class_a:
        a = ClassA(N)
        assert a.distinct(), N
        _class_a[N] = a
    return _class_a[N]


# ---- input class B: rounded values shaped like real spectra ----
class ClassB:
    """seeded normal floats falling off as 1 / (1 + k^2) with the frequency k (in units of N / 16 pixels^-1), a large real
    value at the origin; every product rounds"""

    def __init__(self, N, seed=5):
        rng = np.random.default_rng([N, seed, 2])
        H = N // 2 + 1
        self.N, self.H, self.M = N, H, N * H
        fx = np.minimum(np.arange(N), N - np.arange(N))[:, None] * (16.0 / N)
        fy = np.arange(H)[None, :] * (16.0 / N)
        decay = (1.0 / (1.0 + fx * fx + fy * fy))[None, :, :, None]
        self.proj = (rng.standard_normal((N_ORIENT, N, H, 2)) * decay * N).astype(f32)
        self.ctf = (rng.standard_normal((N_CTF, N, H, 2)) * decay).astype(f32)
        self.proj[:, 0, 0] = [(37.5 * N * (1 + 0.01 * o), 0) for o in range(N_ORIENT)]
        self.ctf[:, 0, 0] = [(1 - 0.03 * c, 0) for c in range(N_CTF)]
        self.ctf_param = np.array([[0.01 * (c + 1), 0.7 + 0.1 * c, 3.0 * c + 1] for c in range(N_CTF)], dtype=f32)
        self.re, self.im, self.mag_re, self.mag_im = conv_exact(self.proj[:, None], self.ctf[None])


_class_b = {}


def class_b(N):
    if N not in _class_b:
        _class_b[N] = ClassB(N)
    return _class_b[N]


def weighted_fsum(conv, N):
    """the sum of x x + y y with the weights 2/1/1 over a float32 spectrum [N, H, 2], correctly rounded to double: a float
    squared has 48 significant bits and is exact in double, as is its double, and math.fsum adds doubles exactly"""
    import math
    bins, weights = parseval_order(N)       # (the order does not matter to an exact sum; the weights go with the bins)
    v = np.asarray(conv, dtype=f32).reshape(-1, 2).astype(f64)[bins]
    w = weights.astype(f64)
    return math.fsum((v[:, 0] * v[:, 0] * w).tolist() + (v[:, 1] * v[:, 1] * w).tolist())
