"""Exact reference of the r2c (fftwf_plan_dft_r2c_2d: forward, unnormalised, out[b][u][k], k < N / 2 + 1) and the word
rule its kernels are held to.  Shares no code with the product: two direct passes in numpy.longdouble over
one table cis[t] = exp(2 pi i t / N) built in mpmath and split into hi + lo; phases are integer products reduced mod N.

The word rule.  Everything between the float input and the float output of the kernels is double, so with
E = m 2^-53 sum|x| (m: rounded operations on the longest path from a pixel to a bin, below) the double a kernel rounds
lies within E of the exact value, and every float word must be the float nearest to a value in [exact - E, exact + E]:
  one answer   both ends of that interval round to the same float: the word is that float, bit for bit
  two answers  a midpoint of two floats lies in the interval: the word is one of the two
  small        |exact| <= E (imaginary parts of self-conjugate bins, cancelled bins): |word| <= E + h, h half a float
               spacing at the exact value
  subnormal    the exact value is below the float normal range: exempt, counted
The share of E a stack PROVES the kernel to have used: for a small word (|word - exact| - h) / E, for a two-answers word
that is not the float nearest the exact value the distance from the exact value to the midpoint it crossed, over E.  (A
one-answer word proves nothing beyond "less than the distance to the next midpoint".)  A share above 1 is a failure.
"""
import functools

import numpy as np

LD = np.longdouble
f32 = np.float32
U53 = LD(2.0) ** -53
F32_TINY = LD(2.0) ** -126


# ---- the table ----
@functools.lru_cache(maxsize=None)
def cis_table(N):
    """(c_hi, c_lo, s_hi, s_lo): cos and sin of 2 pi t / N, t < N, as longdouble hi + double lo (|lo| <= 2^-64 |hi|)"""
    import mpmath
    out = [np.zeros(N, dtype=LD), np.zeros(N), np.zeros(N, dtype=LD), np.zeros(N)]
    with mpmath.workprec(256):
        for t in range(N):
            ang = 2 * mpmath.pi * t / N
            # the exact values where the series would leave 1e-77
            vals = (mpmath.cos(ang), mpmath.sin(ang))
            if (4 * t) % N == 0:
                q = (4 * t) // N
                vals = ((1, 0), (0, 1), (-1, 0), (0, -1))[q]
                vals = (mpmath.mpf(vals[0]), mpmath.mpf(vals[1]))
            for o, v in zip((0, 2), vals):
                hi = LD(mpmath.nstr(v, 45))
                d1 = float(hi)
                d2 = float(hi - LD(d1))                     # hi = d1 + d2 exactly
                out[o][t] = hi
                out[o + 1][t] = float(v - mpmath.mpf(d1) - mpmath.mpf(d2))
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _two_pass(images, c, s, c_lo=None, s_lo=None, round_rows=None):
    """out[b][u][k] = sum_i sum_j x[b][i][j] (c - i s)[(u i + k j) mod N] as a row pass over j and a column pass over i;
    c, s longdouble tables, c_lo, s_lo their double corrections (the products with them need double only)"""
    x = np.asarray(images)
    n, N, _ = x.shape
    H = N // 2 + 1
    jk = (np.arange(N)[:, None] * np.arange(H)[None, :]) % N            # [j][k]
    ui = (np.arange(N)[:, None] * np.arange(N)[None, :]) % N            # [u][i]
    xl = x.astype(LD)
    Rr = xl.reshape(n * N, N) @ c[jk]
    Ri = -(xl.reshape(n * N, N) @ s[jk])
    if c_lo is not None:
        xd = x.astype(np.float64).reshape(n * N, N)
        Rr += (xd @ c_lo[jk]).astype(LD)
        Ri -= (xd @ s_lo[jk]).astype(LD)
    Rr, Ri = Rr.reshape(n, N, H), Ri.reshape(n, N, H)
    if round_rows is not None:
        Rr, Ri = Rr.astype(round_rows).astype(LD), Ri.astype(round_rows).astype(LD)
    Wc, Ws = c[ui], s[ui]
    re = np.empty((n, N, H), dtype=LD)
    im = np.empty((n, N, H), dtype=LD)
    for b in range(n):
        re[b] = Wc @ Rr[b] + Ws @ Ri[b]
        im[b] = Wc @ Ri[b] - Ws @ Rr[b]
        if c_lo is not None:
            rd, idb = Rr[b].astype(np.float64), Ri[b].astype(np.float64)
            re[b] += (c_lo[ui] @ rd + s_lo[ui] @ idb).astype(LD)
            im[b] += (c_lo[ui] @ idb - s_lo[ui] @ rd).astype(LD)
    return re, im


def exact_r2c(images):
    """[n, N, N] float -> (re, im) longdouble [n, N, N // 2 + 1]"""
    images = np.asarray(images)
    assert images.ndim == 3 and images.shape[1] == images.shape[2]
    c, cl, s, sl = cis_table(images.shape[1])
    return _two_pass(images, c, s, cl, sl)


def exact_sparse(N, pixels):
    """the closed form sum_j a_j cis((u y_j + k x_j) mod N) of an image that is zero but for pixels = [(y, x, a), ...]:
    (re, im) longdouble [N, N // 2 + 1]"""
    c, cl, s, sl = cis_table(N)
    H = N // 2 + 1
    u = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(H, dtype=np.int64)[None, :]
    re = np.zeros((N, H), dtype=LD)
    im = np.zeros((N, H), dtype=LD)
    lo_re = np.zeros((N, H))
    lo_im = np.zeros((N, H))
    for y, x, a in pixels:
        t = (u * int(y) + k * int(x)) % N
        a = f32(a)
        re += LD(a) * c[t]
        im -= LD(a) * s[t]
        lo_re += float(a) * cl[t]
        lo_im -= float(a) * sl[t]
    return re + lo_re.astype(LD), im + lo_im.astype(LD)


# ---- the word rule ----
class Verdict:
    def __init__(self, one, two, small, subnormal, bad, share, loose, first_bad):
        self.one, self.two, self.small, self.subnormal, self.bad, self.share = one, two, small, subnormal, bad, share
        self.loose = loose                                  # words classed two answers or small
        self.first_bad = first_bad
        self.words = one + two + small + subnormal

    def __str__(self):
        return "one %d  two %d  small %d  subnormal %d  failing %d  largest share of E %.3f" % (
            self.one, self.two, self.small, self.subnormal, self.bad, self.share)


def words_of(got):
    """complex64 [..., H] or float32 [..., H, 2] -> float32 [..., H, 2]"""
    got = np.asarray(got)
    if got.dtype == np.complex64:
        return got.view(f32).reshape(got.shape + (2,))
    assert got.dtype == f32 and got.shape[-1] == 2
    return got


def verdict(got, exact_re, exact_im, sum_abs, m):
    """classify every float word of `got` against the exact spectrum; sum_abs = sum|x| of the image(s), a scalar or one
    value per leading index"""
    g = words_of(got)
    x = np.stack([np.asarray(exact_re, dtype=LD), np.asarray(exact_im, dtype=LD)], axis=-1)
    assert g.shape == x.shape, (g.shape, x.shape)
    E = LD(m) * U53 * np.asarray(sum_abs, dtype=LD)
    E = E.reshape(E.shape + (1,) * (x.ndim - E.ndim))
    E = np.broadcast_to(E, x.shape)
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        lo, hi, near = (x - E).astype(f32), (x + E).astype(f32), x.astype(f32)
        h = np.spacing(np.abs(near)).astype(LD) / 2
        small = ax <= E
        sub = ~small & (ax < F32_TINY)
        one = ~small & ~sub & (lo == hi)
        two = ~small & ~sub & (lo != hi)
        gl = g.astype(LD)
        ok = np.where(small, np.abs(gl) <= E + h, (g >= lo) & (g <= hi)) | sub
        share_small = np.where(small, (np.abs(gl - x) - h) / E, 0)
        crossed = two & (g != near)
        share_two = np.where(crossed, np.abs(x - (near.astype(LD) + gl) / 2) / E, 0)
        share = float(max(share_small.max(initial=0), share_two.max(initial=0), 0))
    bad = ~ok
    return Verdict(int(one.sum()), int(two.sum()), int(small.sum()), int(sub.sum()), int(bad.sum()), share, small | two,
                   np.argwhere(bad)[:5])


# ---- the kernel selection and m, restated from the launchers ----
MAX_LEN = 20          # compiled sub-transform lengths of the fast transform: 2 ... 20
MFMA_MAX_N = 304
TW_LDS_MAX_N = 3072


def split(N):
    A = 1
    d = 1
    while d * d <= N:
        if N % d == 0:
            A = d
        d += 1
    return A, N // A


def family(N, dft=False):
    """the kernel pair a transform of N x N images takes: dft = under BIOEM_R2C=dft"""
    A, B = split(N)
    if not dft and N >= 4 and A >= 2 and B <= MAX_LEN:
        return "fft16" if B <= 16 else "fft20"
    if N <= MFMA_MAX_N and A * ((B + 15) // 16) <= 40:
        return "mfma2" if A * ((B + 15) // 16) <= 16 else "mfma5"
    return "dft_lds" if N <= TW_LDS_MAX_N else "dft_global"


def fft_plan(N):
    """G (transforms per block iteration) and blocks per CU of k_r2c_fft, as r2c_fft_plan / bioem_r2c_fft_launch"""
    A, B = split(N)
    raw = A * (B + 1)
    YG = raw + (B - raw) % 32
    G = 256 // B
    while True:
        Gp = G | 1
        plane = max(G * YG, N * Gp)
        lds = 8 * (2 * N + 2 * plane)
        if lds <= 53 * 1024 or G == 1:
            break
        G -= 1
    return G, max(1, min(4, 160 * 1024 // (lds + 512)))


def units_and_grid(N, n_img, n_cu, dft=False):
    """[(units, blocks)] of the row and the column launch of the resident-grid kernels"""
    fam = family(N, dft)
    H = N // 2 + 1
    if fam.startswith("fft"):
        G, per_cu = fft_plan(N)
        units = [-(-n_img * ((N + 1) // 2) // G), -(-n_img * H // G)]
    else:
        assert fam.startswith("mfma")
        per_cu = max(1, min(4, 160 * 1024 // (N * (16 + 2 * 17 * 8) + 1024))) if fam == "mfma2" else 1
        units = [((N + 15) // 16) * n_img, ((H + 15) // 16) * n_img]
    return [(u, min(u, per_cu * n_cu)) for u in units]


def _radix(L):
    if L % 4 == 0:
        return 4
    for p in range(2, L):
        if L % p == 0:
            return p
    return L


def _fft_depth(L):
    """rounded operations a value passes in r2c_fft_fwd<L>.  Butterfly of 2: one add.  Of 4: two adds.  Of an odd P,
    Q = (P - 1) / 2: one add (a = t[q+1] + t[P-1-q]), a chain of Q fma with constants of the CIS table (2 for their
    error), one add (e -+ i f): Q + 4.  Between the levels the twiddle of the CIS table: one multiply, one fma, 2 for
    the constant: 4 (the trivial twiddles cost nothing; the longest path takes a real one)."""
    if L == 1:
        return 0
    P = _radix(L)
    bf = 1 if P == 2 else 2 if P == 4 else (P - 1) // 2 + 4
    return bf if L == P else _fft_depth(L // P) + 4 + bf


def m(path, A, B):
    """rounded operations on the longest path from an input pixel to an output bin; an add, a multiply or an fma counts
    1, a twiddle read from a table 2 for its own error (the table entry is cos / sin of an angle rounded twice).

    "dft" (k_dft_rows / k_dft_cols): the row pass runs a chain of B fma over the real inputs (a pixel at j2 = 0 passes
    all of them) with a table twiddle, B + 2, then A terms of two fma each on both components, 2 A + 2; the column pass
    has complex inputs in both stages, 2 B + 2 and 2 A + 2: 3 B + 4 A + 8.

    "mfma" (k_dft_*_mfma): the same sums as instructions of four products; each product counts as one rounded add and a
    chain of L terms takes ceil(L / 4) instructions, so L is rounded up to L4 = 4 ceil(L / 4): 3 B4 + 4 A4 + 8.

    "fft" (k_r2c_fft): per pass the FFT of B points, the table twiddle w_N^(j1 kb) (multiply, fma, 2: 4) and the FFT of
    A points; the row pass adds the separation of the two rows, 0.5 (z + conj z'): one add (the halving is exact).
    2 (depth(A) + depth(B)) + 9 with depth as _fft_depth.

    The rounding to float at the end is what the rule tests and is not counted.  None exceeds 4 (A + B) + 32."""
    if path == "dft":
        v = 3 * B + 4 * A + 8
    elif path == "mfma":
        v = 3 * (4 * -(-B // 4)) + 4 * (4 * -(-A // 4)) + 8
    else:
        assert path == "fft"
        v = 2 * (_fft_depth(A) + _fft_depth(B)) + 9
    assert v <= 4 * (A + B) + 32
    return v


def m_of(N, dft=False):
    fam = family(N, dft)
    return m("fft" if fam.startswith("fft") else "mfma" if fam.startswith("mfma") else "dft", *split(N))


# ---- sums ----
def seq_sums(image):
    """sequential float32 sum and sum of squares in row-major order, the square rounded before it is added (no fma):
    k_map_sums, bioem.cpp:2087-2107"""
    v = np.ascontiguousarray(image, dtype=f32).reshape(-1)
    sq = v * v
    assert sq.dtype == f32
    return np.add.accumulate(v, dtype=f32)[-1], np.add.accumulate(sq, dtype=f32)[-1]


# ---- inputs ----
def sparse_pixels(N, seed):
    """one pixel per row and per column, (i, perm(i)); amplitudes multiples of 1/16 in [0.5, 2] (25 values, each used
    once before any is used again): every sum of amplitudes is an exact float"""
    rng = np.random.default_rng([N, seed, 1])
    perm = rng.permutation(N)
    amps = np.concatenate([rng.permutation(np.arange(8, 33)) for _ in range(-(-N // 25))])[:N] / 16.0
    return [(i, int(perm[i]), float(amps[i])) for i in range(N)]


def image_of(N, pixels, transpose=False):
    img = np.zeros((N, N), dtype=f32)
    for y, x, a in pixels:
        img[(x, y) if transpose else (y, x)] = a
    return img


def dense_image(N, seed):
    return np.random.default_rng([N, seed, 2]).integers(-8, 9, (N, N)).astype(f32)


def wide_image(N, seed):
    rng = np.random.default_rng([N, seed, 3])
    return (rng.standard_normal((N, N)) * np.exp(3 * rng.standard_normal((N, N)))).astype(f32)


KINDS = ("sparse", "dense", "sparse_t", "dense", "sparse")


@functools.lru_cache(maxsize=None)
def case_image(N, j):
    """image j of size N and its exact spectrum: j = 0, 1, 2 are sparse, dense, sparse transposed; from 3 on dense and
    sparse alternate.  Returns (image, re, im, sum|x|), all read-only"""
    kind = KINDS[j] if j < len(KINDS) else ("dense", "sparse")[j % 2]
    if kind == "dense":
        img = dense_image(N, j)
        re, im = exact_r2c(img[None])
        re, im = re[0], im[0]
    else:
        px = sparse_pixels(N, j)
        if kind == "sparse_t":
            px = [(x, y, a) for y, x, a in px]
        img = image_of(N, px)
        re, im = exact_sparse(N, px)
    out = (img, re, im, LD(np.abs(img.astype(np.float64)).sum()))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def case_stack(N, n=3):
    """(images [n, N, N], re, im, sum|x| [n]) of images 0 ... n - 1"""
    parts = [case_image(N, j) for j in range(n)]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
            np.array([p[3] for p in parts], dtype=LD))


def big_sparse(N=3080, n_pix=8, seed=5):
    """8 pixels of a 3080 x 3080 image, rows and columns all distinct and spread over the residues of 55 and 56"""
    rng = np.random.default_rng([N, seed, 4])
    ys, xs = rng.permutation(N)[:n_pix], rng.permutation(N)[:n_pix]
    amps = rng.permutation(np.arange(8, 33))[:n_pix] / 16.0
    return [(int(y), int(x), float(a)) for y, x, a in zip(ys, xs, amps)]


# the sizes of tests/test_r2c_exact_gpu.py, shared with the host test that holds the reference to the caps
SQUARES = [L * L for L in range(2, 21)]
SIZES_A = sorted(set(SQUARES + [6, 20, 35, 380, 256, 272, 289]))
SIZES_A_DFT = [N for N in SIZES_A if N <= 100 or N == 289]
RAGGED = [(16, 1), (16, 2), (16, 5), (35, 1), (35, 2), (35, 5)]
SIZES_B = [23, 46, 207, 305]            # default path
SIZES_B_DFT = [153]
HANDOVER = {
    # N: (under BIOEM_R2C=dft, distinct images)
    16: (False, 64), 20: (False, 64), 289: (False, 4), 23: (False, 16), 153: (True, 4),
}
HANDLE_SIZES = [35, 64, 256]
SUM_SIZES = [63, 64, 65, 91, 128]
