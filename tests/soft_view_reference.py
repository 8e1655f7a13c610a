"""Reference of the posterior-weighted view sums (bioem_hip_view_sums_soft, bioem_hip_debug_view_sums_soft); shares no code
with the product.

A member r = (particle p, group g, CTF set c) carries a table a_r[i][j] over the cells (X_i, X_j) of a shift list and the
scalars s2_r, b_r, mass_r.  With R_p, K~_c and tw(j) = exp(+2 pi i j / N) as in tests/view_reference.py:

    W_r[k1][k2] = sum_i sum_j a_r[i][j] tw((k1 X_i + k2 X_j) mod N)
    num_g[k] = sum_r K~_c[k] (R_p[k] W_r[k] - [k = 0] b_r N^2)          den_g[k] = sum_r s2_r |K~_c[k]|^2

exact_sums forms these in integers in the manner of view_reference.exact_sums: every float32 / float64 input is a dyadic
rational and enters exactly (the doubles a, s2, b as multiples of 2^-D_BITS, which to_int checks), a twiddle enters as the
integer nearest to 2^160 times its value, W as the product of the two twiddles of a cell, so a sum is exact up to 2^-159 of
its terms; it comes back as (hi, lo) float64 pairs.  numpy_sums restates the definition in plain float64, one cell at a
time.  brute_force gives the nd^2 pseudo-particles per member, one per cell, on which view_reference.numpy_sums computes
the same sums.  scales gives the quantity the bound of DESIGN 2.22 multiplies:

    |num - exact| <= (C_NUM + 2 nd + n_g) 2^-53 sum_r |K~| (|R| sum_cells |a| + |b| N^2 [k = 0])        per component
    |den - exact| <= (C_DEN + n_g) 2^-53 sum_r s2 |K~|^2

C_NUM = 16 counts the roundings of one term of the arithmetic of soft_kernels.hpp, in modulus and in units of 2^-53: the
two twiddle tables (each component within 1 ulp of 1: 2 each, rounded up from sqrt 2), the real x complex product a tw of
the column pass (1), the complex product tw U of the row pass (sqrt 5 < 2.24), the complex product R W (2.24), b N^2 and
its subtraction (1 + 1, on their own part of the scale), the sum of the two kernels in a self-conjugate column (sqrt 2 <
1.42), the last complex product (2.24): 4 + 1 + 2.24 + 2.24 + 2 + 1.42 + 2.24 = 15.14 < 16.  2 nd: the nd - 1 additions of
each of the two passes, one rounding each against a partial sum of at most sum |a|.  n_g: one rounding per addition of the
accumulation.  C_DEN = 8 as in view_reference (s2 is handed in: two roundings fewer)."""
import fractions

import numpy as np

import view_reference as vr

C_NUM = 16.0
C_DEN = 8.0
U = vr.U
D_BITS = 200  # every double of the tests times 2^D_BITS is an integer


def _hermitian_int(ctf_c, N):
    """2 K~ of a complex kernel [N][H], exactly, as two object arrays of integers at 2^F32_BITS"""
    kr, ki = 2 * vr.to_int(ctf_c.real, vr.F32_BITS), 2 * vr.to_int(ctf_c.imag, vr.F32_BITS)
    partner = (-np.arange(N)) % N
    for col in ([0, N // 2] if N % 2 == 0 else [0]):
        kr[:, col], ki[:, col] = (kr[:, col] + kr[partner, col]) // 2, (ki[:, col] - ki[partner, col]) // 2
    return kr, ki


def member_order(members, g):
    """the members of group g in the order of the additions: ascending (particle, position in the list)"""
    idx = [r for r in range(len(members)) if int(members[r]["group"]) == g]
    return sorted(idx, key=lambda r: (int(members[r]["particle"]), r))


def exact_sums(spec, ctf, members, cells, shifts, n_groups):
    """num_hi, num_lo complex128 [nG][N][H]; den_hi, den_lo float64 [nG][N][H]; stats float64 [nG][2] (count and the
    correctly rounded sum of the masses)"""
    spec, ctf = vr.as_complex(spec), vr.as_complex(ctf)
    _, N, H = spec.shape
    X = [int(x) for x in np.asarray(shifts).reshape(-1)]
    nd = len(X)
    cells = np.asarray(cells, dtype=np.float64).reshape(len(members), nd, nd)
    tc, ts = vr.twiddles_int(N)
    k1 = np.arange(N, dtype=np.int64)
    k2 = np.arange(H, dtype=np.int64)
    rowc = [tc[(k1 * x) % N] for x in X]   # [nd] of object [N]
    rows = [ts[(k1 * x) % N] for x in X]
    colc = [tc[(k2 * x) % N] for x in X]   # [nd] of object [H]
    cols = [ts[(k2 * x) % N] for x in X]
    Kint, Rint = {}, {}
    out = [np.zeros((n_groups, N, H), dtype=np.complex128) for _ in range(2)] + \
          [np.zeros((n_groups, N, H), dtype=np.float64) for _ in range(2)]
    stats = np.zeros((n_groups, 2))
    Sn = 2 * vr.F32_BITS + 1 + D_BITS + 2 * vr.TW_BITS   # (the kernel entered doubled)
    Sd = 2 * vr.F32_BITS + 2 + D_BITS
    for g in range(n_groups):
        order = member_order(members, g)
        stats[g, 0] = len(order)
        sm = sum((fractions.Fraction(float(members[r]["mass"])) for r in order), fractions.Fraction(0))
        stats[g, 1] = sm.numerator / sm.denominator
        if not order:
            continue
        sr = si = sd = 0
        for r in order:
            m = members[r]
            p, c = int(m["particle"]), int(m["conv"])
            if c not in Kint:
                Kint[c] = _hermitian_int(ctf[c], N)
            if p not in Rint:
                Rint[p] = (vr.to_int(spec[p].real, vr.F32_BITS), vr.to_int(spec[p].imag, vr.F32_BITS))
            kr, ki = Kint[c]
            xr, xi = Rint[p]
            a = vr.to_int(cells[r], D_BITS)
            # U[i][k2] = sum_j a[i][j] tw(k2 X_j), W[k1][k2] = sum_i tw(k1 X_i) U[i][k2]: exact, so in any order
            wr = np.zeros((N, H), dtype=object)
            wi = np.zeros((N, H), dtype=object)
            for i in range(nd):
                ur = sum((int(a[i, j]) * colc[j] for j in range(nd) if a[i, j]), np.zeros(H, dtype=object))
                ui = sum((int(a[i, j]) * cols[j] for j in range(nd) if a[i, j]), np.zeros(H, dtype=object))
                wr = wr + (rowc[i][:, None] * ur[None, :] - rows[i][:, None] * ui[None, :])
                wi = wi + (rowc[i][:, None] * ui[None, :] + rows[i][:, None] * ur[None, :])
            ar, ai = xr * wr - xi * wi, xr * wi + xi * wr
            ar[0, 0] -= (vr.to_int(np.float64(m["b"]), D_BITS).item() * N * N) << (vr.F32_BITS + 2 * vr.TW_BITS)
            sr = sr + (kr * ar - ki * ai)
            si = si + (kr * ai + ki * ar)
            sd = sd + (kr * kr + ki * ki) * vr.to_int(np.float64(m["s2"]), D_BITS).item()
        for a1 in range(N):
            for a2 in range(H):
                rh, rl = vr._round_pair(int(sr[a1, a2]), Sn)
                ih, il = vr._round_pair(int(si[a1, a2]), Sn)
                out[0][g, a1, a2], out[1][g, a1, a2] = complex(rh, ih), complex(rl, il)
                out[2][g, a1, a2], out[3][g, a1, a2] = vr._round_pair(int(sd[a1, a2]), Sd)
    return out[0], out[1], out[2], out[3], stats


def numpy_sums(spec, ctf, members, cells, shifts, n_groups):
    """the definition in float64, one cell at a time: (num complex128 [nG][N][H], den float64 [nG][N][H], stats [nG][2])"""
    spec, ctf = vr.as_complex(spec), vr.as_complex(ctf)
    _, N, H = spec.shape
    X = [int(x) for x in np.asarray(shifts).reshape(-1)]
    nd = len(X)
    cells = np.asarray(cells, dtype=np.float64).reshape(len(members), nd, nd)
    num = np.zeros((n_groups, N, H), dtype=np.complex128)
    den = np.zeros((n_groups, N, H))
    stats = np.zeros((n_groups, 2))
    for g in range(n_groups):
        for r in member_order(members, g):
            m = members[r]
            W = np.zeros((N, H), dtype=np.complex128)
            for i in range(nd):
                for j in range(nd):
                    if cells[r, i, j]:
                        W += cells[r, i, j] * np.exp(2j * np.pi * vr.shift_index(N, X[i], X[j]) / N)
            A = spec[int(m["particle"])] * W
            A[0, 0] -= float(m["b"]) * N * N
            K = vr.hermitian_kernel(ctf[int(m["conv"])])
            num[g] += K * A
            den[g] += float(m["s2"]) * np.abs(K) ** 2
            stats[g] += (1.0, float(m["mass"]))
    return num, den, stats


def brute_force(spec, members, cells, cell_mu, shifts):
    """(spectra, records, group_of) of the nd^2 pseudo-particles per member, one per cell, for view_reference.numpy_sums at
    weight 1: norm = a (a float32 value), the cell's mu, the cell's shift; the member then has b = sum a mu and s2 = sum
    a^2.  Records carry the fields numpy_sums reads."""
    spec = vr.as_complex(spec)
    X = [int(x) for x in np.asarray(shifts).reshape(-1)]
    nd = len(X)
    dt = np.dtype([("cent_x", "<i4"), ("cent_y", "<i4"), ("conv", "<i4"), ("norm", "<f4"), ("mu", "<f4")])
    S, rec, grp = [], [], []
    for r, m in enumerate(members):
        for i in range(nd):
            for j in range(nd):
                a = np.float32(cells[r][i][j])
                assert float(a) == float(cells[r][i][j]), "a is no float32 value"
                S.append(spec[int(m["particle"])])
                rec.append((X[i], X[j], int(m["conv"]), a, np.float32(cell_mu[r][i][j])))
                grp.append(int(m["group"]))
    return np.array(S), np.array(rec, dtype=dt), np.array(grp, dtype=np.int32)


def scales(spec, ctf, members, cells, n_groups):
    """(sum_r |term_r| of num, of den) float64 [nG][N][H] each, and the group sizes"""
    spec, ctf = vr.as_complex(spec), vr.as_complex(ctf)
    _, N, H = spec.shape
    cells = np.asarray(cells, dtype=np.float64).reshape(len(members), -1)
    an = np.zeros((n_groups, N, H))
    ad = np.zeros((n_groups, N, H))
    size = np.zeros(n_groups, dtype=np.int64)
    for r, m in enumerate(members):
        g = int(m["group"])
        if g < 0:
            continue
        mag = np.abs(spec[int(m["particle"])]) * np.abs(cells[r]).sum()
        mag[0, 0] += abs(float(m["b"])) * N * N
        K = np.abs(vr.hermitian_kernel(ctf[int(m["conv"])]))
        an[g] += K * mag
        ad[g] += float(m["s2"]) * K ** 2
        size[g] += 1
    return an, ad, size


def bounds(an, ad, size, nd):
    """the derived bounds per coefficient: (num per component, den)"""
    n = size.astype(np.float64)[:, None, None]
    return (C_NUM + 2.0 * nd + n) * U * an, (C_DEN + n) * U * ad


errors = vr.errors


def ratios(err, bound):
    """err / bound per coefficient, inf where a zero bound is exceeded"""
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))


def device_twiddles(N):
    """(cos, sin) float64 [N] of the table the kernels read: the library's values, 0 and +-1 where 4 j is a multiple of N"""
    j = np.arange(N)
    c, s = np.cos(2.0 * np.pi * j / N), np.sin(2.0 * np.pi * j / N)
    q = np.flatnonzero((4 * j) % N == 0)
    c[q] = np.array([1.0, 0.0, -1.0, 0.0])[(4 * q // N) % 4]
    s[q] = np.array([0.0, 1.0, 0.0, -1.0])[(4 * q // N) % 4]
    return c, s


def ordered_sums(spec, ctf, members, cells, shifts, n_groups):
    """the arithmetic of soft_kernels.hpp restated in float64, every product and sum rounded once in the stated order (real
    arrays: nothing is fused): (num complex128 [nG][N][H], den float64 [nG][N][H])"""
    spec, ctf = vr.as_complex(spec), vr.as_complex(ctf)
    _, N, H = spec.shape
    X = [int(x) % N for x in np.asarray(shifts).reshape(-1)]
    nd = len(X)
    cells = np.asarray(cells, dtype=np.float64).reshape(len(members), nd, nd)
    tc, ts = device_twiddles(N)
    k1, k2 = np.arange(N), np.arange(H)
    partner = (-k1) % N
    self_cols = [0, N // 2] if N % 2 == 0 else [0]
    num = np.zeros((n_groups, N, H), dtype=np.complex128)
    den = np.zeros((n_groups, N, H))
    for g in range(n_groups):
        nr, ni, dn = np.zeros((N, H)), np.zeros((N, H)), np.zeros((N, H))
        for r in member_order(members, g):
            m = members[r]
            a = cells[r]
            ur, ui = np.zeros((nd, H)), np.zeros((nd, H))
            for j in range(nd):
                t = (k2 * X[j]) % N
                ur = ur + a[:, j, None] * tc[t][None, :]
                ui = ui + a[:, j, None] * ts[t][None, :]
            wr, wi = np.zeros((N, H)), np.zeros((N, H))
            for i in range(nd):
                t = (k1 * X[i]) % N
                wr = wr + (tc[t][:, None] * ur[i][None, :] - ts[t][:, None] * ui[i][None, :])
                wi = wi + (tc[t][:, None] * ui[i][None, :] + ts[t][:, None] * ur[i][None, :])
            R = spec[int(m["particle"])]
            xr, xi = R.real.copy(), R.imag.copy()
            ar = xr * wr - xi * wi
            ai = xr * wi + xi * wr
            ar[0, 0] = ar[0, 0] - float(m["b"]) * (float(N) * float(N))
            K = ctf[int(m["conv"])]
            hx, hy = K.real.copy(), K.imag.copy()
            for col in self_cols:
                hx[:, col] = 0.5 * (K.real[:, col] + K.real[partner, col])
                hy[:, col] = 0.5 * (K.imag[:, col] - K.imag[partner, col])
            nr = nr + (hx * ar - hy * ai)
            ni = ni + (hx * ai + hy * ar)
            dn = dn + float(m["s2"]) * (hx * hx + hy * hy)
        num[g], den[g] = nr + 1j * ni, dn
    return num, den


MEMBER_DTYPE = np.dtype([("particle", "<i4"), ("group", "<i4"), ("conv", "<i4"), ("pad", "<i4"), ("s2", "<f8"), ("b", "<f8"),
                         ("mass", "<f8")])


def shift_list(N, nd):
    """nd shifts in (-N, N) with both ends, 0 and a repeated value as far as nd allows; neither sorted nor distinct"""
    base = [-(N - 1), N - 1, 3, 3, 0] + [((7 * k) % (2 * N - 1)) - (N - 1) for k in range(1, N)]
    return np.array(base[:nd], dtype=np.int32)


def random_complex(n, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    return (scale * (rng.standard_normal((n, N, H)) + 1j * rng.standard_normal((n, N, H)))).astype(np.complex64)


def rounded_problem(N, nd, nCTF, seed):
    """(spectra complex64 [5, N, H], members, cells, shifts, nGroups) of the rounded class: four groups of 4, 1, 0 and 2
    members, a particle with two CTF sets in one group and in a second group, a member left out; tables of mixed sign whose
    sum nearly cancels (W at k = 0, and wherever the shifts' twiddles line up), one all-positive table, one one-hot table;
    b of either sign up to 1e3"""
    rng = np.random.default_rng(seed)
    spec = random_complex(5, N, seed + 1, 3.0)
    shifts = shift_list(N, nd)
    plan = [(0, 0, 0), (1, 0, 1), (1, 0, 2), (2, 0, 3), (3, 1, 1), (0, 3, 2), (4, 3, 0), (2, -1, 0), (1, 3, 1)]
    mem = np.zeros(len(plan), dtype=MEMBER_DTYPE)
    cells = np.zeros((len(plan), nd, nd))
    for r, (p, g, c) in enumerate(plan):
        mem[r]["particle"], mem[r]["group"], mem[r]["conv"] = p, g, c % nCTF
        a = rng.standard_normal((nd, nd))
        if nd > 1 and r % 3 != 1:
            a = a - a.mean() + 1e-13 * rng.standard_normal()   # nearly cancelling
        if r == 4:
            a = np.abs(a) + 0.25
        if r == 5:
            a = np.zeros((nd, nd))
            a[nd // 2, nd - 1] = -1.75
        cells[r] = a
        mem[r]["s2"] = rng.random() * 3.0
        mem[r]["b"] = rng.standard_normal() * (1.0e3 if r % 2 else 1.0)
        mem[r]["mass"] = rng.random()
    return spec, mem, cells, shifts, 4


def exact_problem(nd, sizes, nCTF, seed, N=32):
    """the exact class: shifts from {0, +-8, +-16} at N = 32 (twiddles 1, i, -1, -i), small-integer spectra, tables and
    scalars, so every product and sum of the kernels is exact.  sizes: members per group; member k of group g is of
    particle (k + g) mod (nSpec - 1), so particles sit in several groups, the last particle has no member, and the list is
    shuffled.  Returns (spectra, members, cells, shifts, nGroups)."""
    rng = np.random.default_rng(seed)
    nG = len(sizes)
    nSpec = max(sizes) + 2
    H = N // 2 + 1
    spec = (rng.integers(-8, 9, (nSpec, N, H)) + 1j * rng.integers(-8, 9, (nSpec, N, H))).astype(np.complex64)
    shifts = np.array([0, 8, -16, -8, 16][:nd], dtype=np.int32)
    plan = [((k + g) % (nSpec - 1), g) for g, s in enumerate(sizes) for k in range(s)]   # particle nSpec - 1: no member
    order = rng.permutation(len(plan))
    mem = np.zeros(len(plan), dtype=MEMBER_DTYPE)
    cells = rng.integers(-4, 5, (len(plan), nd, nd)).astype(np.float64)
    for r, k in enumerate(order):
        mem[r]["particle"], mem[r]["group"] = plan[k]
        mem[r]["conv"] = int(rng.integers(0, nCTF))
        mem[r]["s2"] = float(rng.integers(0, 6))
        mem[r]["b"] = float(rng.integers(-3, 4))
        mem[r]["mass"] = float(rng.integers(0, 3)) * 0.25
    return spec, mem, cells, shifts, nG


def integer_kernels(nCTF, N, seed):
    rng = np.random.default_rng(seed)
    H = N // 2 + 1
    return (rng.integers(-4, 5, (nCTF, N, H)) + 1j * rng.integers(-4, 5, (nCTF, N, H))).astype(np.complex64)
