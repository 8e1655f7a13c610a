"""Reference of the gradient with respect to the voxels of a volume model (vgrad_kernels.hpp), in numpy double
arithmetic, one rounding per written operation.  It shares no code with the library and does not call it; the rotation
matrix is the float32 one of tests/projection_reference.py, widened.

    Y = prepare_y(G, N, w, shiftX, shiftY, full)       Y of a stack of spectra [n, N, H], the kernel's expressions
    t = forward_taps(N, pad, R)                        the taps of k_slice_project in its own loop: every stored coefficient
                                                       of the disc, taps t = 0 ... 7, with the forward's q, c, f, g
    g = gather_taps(N, pad, R)                         the same set found from the voxels' side, by the kernel's half-width
                                                       rule (view_parameters): what k_vgrad_insert enumerates
    b = backproject(Y, N, pad, Rs)                     A: the forward taps' terms scattered per voxel and added in the
                                                       kernel's order (b.seq) and with math.fsum (b.fsum), and what the
                                                       bound needs (b.count, b.abs_re, b.abs_im, b.slack)
    insert_bound(b)                                    |device - b.fsum| per component, derived below before anything ran
    adjoint_volume(A, N, pad, centre, precorrect)      gvol from A: un-centring, the three passes, the real part, sinc^2

The bound of the back-insertion, in the form of slice_reference.slice_bound.  A term ((w0 w1) w2) y carries the rounding
of g = 1 - f (f = q - floor(q) is exact), two in the products of the weights and one in the product with y: c = 4.  T_s
terms added in sequence are within T_s u sum|term| of their exact sum.  A coordinate q_j = P ((a R0j) + (b R1j)) takes two
products and a sum, so any evaluation stays within dq = 3 u P max_j (|a| |R0j| + |b| |R1j|) of this one; a weight factor is
piecewise linear with slope at most 1 and at most 1, so a term moves by at most 3 dq (|Re y| + |Im y|):
    |got - fsum| <= (T_s + 4) u sum|term| + 3 sum_terms dq (|Re y| + |Im y|)      per component and voxel.
Y itself is formed here by the kernel's expressions from the twiddle table the library builds (libm's cos and sin of the
reduced index): the same bits.

The passes back to the volume (adjoint_bound): the un-centring is four complex products, each with three roundings per
component and a table entry within u of its value, 20 u |A| per component (slice_reference's C_STORE); a pass of n terms by
fma in sequence is within (n + 2) u sum|term| (one rounding per fma, two per product it replaces, a twiddle within u); the
three passes have PN, PN and PH terms and their errors pass through the later ones with factors of modulus 1.  Every
partial sum is at most sum_k (|Re| + |Im|) of A, so |got - exact| <= 8 (PN + 16) u sum_k (|Re A_k| + |Im A_k|) per voxel,
the form of DESIGN 2.24's spectrum bound, before the division by the sinc^2 product (which multiplies bound and value
alike and adds 3 u)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from projection_reference import rotation_matrix  # noqa: E402

U = 2.0 ** -53
C_TERM = 4
HALF_CAP = 4.0          # kVgradHalfCap
SLACK = 2.0 ** -20
SQRT3 = 1.7320508075688772


def conventions(N, pad):
    PN = pad * N
    return dict(H=N // 2 + 1, o=(N + 1) // 2, M=(N - 1) // 2, PN=PN, PH=PN // 2 + 1, MP=(PN - 1) // 2)


def matrix(angle, is_quat=True):
    return rotation_matrix(np.asarray(angle, dtype=np.float32), is_quat).astype(np.float64)


def twiddle_table(N):
    """exp(+2 pi i j / N) with libm's cos and sin of 2 pi j / N, as the library's host code builds its tables"""
    return np.array([complex(math.cos(2.0 * math.pi * float(j) / float(N)), math.sin(2.0 * math.pi * float(j) / float(N)))
                     for j in range(N)])


def stored(N):
    i = np.arange(N)
    return np.where(i <= N // 2, i, i - N), np.arange(N // 2 + 1)


def twiddle_index(A, B, N, shiftX, shiftY):
    o = (N + 1) // 2
    return (-o * (A + B) + shiftX * A + shiftY * B) % N


def symmetrise(G):
    """Gamma of spectra [..., N, H]: the Hermitian part in column 0"""
    G = np.array(G, dtype=np.complex128)
    N = G.shape[-2]
    mirror = (-np.arange(N)) % N
    col = G[..., :, 0]
    m = col[..., mirror]
    G[..., :, 0] = (col.real + m.real) * 0.5 + 1j * ((col.imag - m.imag) * 0.5)
    return G


def prepare_y(G, N, w=None, shiftX=0, shiftY=0, full=True):
    G = np.asarray(G, dtype=np.complex128)
    n = G.shape[0]
    H, M = N // 2 + 1, (N - 1) // 2
    a, b = stored(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    disc = A * A + B * B <= M * M
    t = twiddle_table(N)[twiddle_index(A, B, N, shiftX, shiftY)]
    v = symmetrise(G) if full else G
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    wb = np.where(B == 0, 1.0, 2.0)
    sc = (w[:, None, None] * wb[None]) / (float(N) * float(N)) if full else w[:, None, None] * np.ones((1, N, H))
    zr = v.real * t.real + v.imag * t.imag
    zi = v.imag * t.real - v.real * t.imag
    return np.where(disc[None], sc * zr + 1j * (sc * zi), 0.0)


class Taps:
    pass


def forward_taps(N, pad, R):
    """the taps of k_slice_project that count, in its own loop order (coefficients in stored order, taps ascending): flat
    arrays vox (the stored voxel's flat index in [PN, PN, PH]), neg, a, b (signed a), wt, dq"""
    cv = conventions(N, pad)
    PN, PH, MP, M = cv["PN"], cv["PH"], cv["MP"], cv["M"]
    R = np.asarray(R, dtype=np.float64)
    a, b = stored(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    A, B = A.ravel(), B.ravel()
    disc = A * A + B * B <= M * M
    A, B = A[disc], B[disc]
    da, db, dp = A.astype(np.float64), B.astype(np.float64), float(pad)
    out = Taps()
    vox, neg, aa, bb, wt, dq = [], [], [], [], [], []
    with np.errstate(all="ignore"):
        q = [dp * ((da * R[0, j]) + (db * R[1, j])) for j in range(3)]
        ok = (np.abs(q[0]) < PN) & (np.abs(q[1]) < PN) & (np.abs(q[2]) < PN)
        q = [np.where(ok, x, 0.0) for x in q]
        c = [np.floor(x) for x in q]
        f = [x - y for x, y in zip(q, c)]
        g = [1.0 - x for x in f]
        i = [x.astype(np.int64) for x in c]
        slack = 3 * U * pad * np.max([np.abs(da) * abs(R[0, j]) + np.abs(db) * abs(R[1, j]) for j in range(3)], axis=0)
        for t in range(8):
            d = (t >> 2, (t >> 1) & 1, t & 1)
            k = [i[j] + d[j] for j in range(3)]
            inside = ok.copy()
            for j in range(3):
                inside &= (k[j] >= -MP) & (k[j] <= MP)
            ng = k[2] < 0
            s = [np.where(ng, -x, x) for x in k]
            w = ((f[0] if d[0] else g[0]) * (f[1] if d[1] else g[1])) * (f[2] if d[2] else g[2])
            flat = ((s[0] % PN) * PN + (s[1] % PN)) * PH + s[2]
            vox.append(flat[inside])
            neg.append(ng[inside])
            aa.append(A[inside])
            bb.append(B[inside])
            wt.append(w[inside])
            dq.append(slack[inside])
    out.vox, out.neg, out.a, out.b = np.concatenate(vox), np.concatenate(neg), np.concatenate(aa), np.concatenate(bb)
    out.wt, out.dq = np.concatenate(wt), np.concatenate(dq)
    return out


def view_parameters(R, pad):
    """what k_vgrad_views forms: (G^-1 / P entries m00, m01, m11, half-widths ha, hb, unit normal, flag)"""
    R = np.asarray(R, dtype=np.float64)
    r0, r1 = R[0], R[1]
    dp = float(pad)
    with np.errstate(all="ignore"):
        g00 = (r0[0] * r0[0] + r0[1] * r0[1]) + r0[2] * r0[2]
        g01 = (r0[0] * r1[0] + r0[1] * r1[1]) + r0[2] * r1[2]
        g11 = (r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]
        det = g00 * g11 - g01 * g01
        flag = 0
        if not (g00 > 0.0) or not (g11 > 0.0) or not (det > 1e-6 * (g00 * g11)) or not (det < 1e300):
            return dict(flag=1)
        i00, i01, i11 = g11 / det, -g01 / det, g00 / det
        ha = (SQRT3 * math.sqrt(i00) / dp) * (1.0 + SLACK) + SLACK
        hb = (SQRT3 * math.sqrt(i11) / dp) * (1.0 + SLACK) + SLACK
        if not (ha <= HALF_CAP and hb <= HALF_CAP):
            flag = 2
    return dict(flag=flag, m00=i00 / dp, m01=i01 / dp, m11=i11 / dp, ha=ha, hb=hb)


def gather_taps(N, pad, R):
    """the taps found from the voxels' side as k_vgrad_insert finds them: for every stored voxel it can reach and each
    target, the candidates (a, b) of the half-width rule, kept iff target - floor(q) is in {0, 1}^3 under the forward's q.
    Flat arrays as forward_taps, in the kernel's order (voxel, target, a, b); None for a view the entries refuse."""
    cv = conventions(N, pad)
    PN, PH, MP, M = cv["PN"], cv["PH"], cv["MP"], cv["M"]
    R = np.asarray(R, dtype=np.float64)
    V = view_parameters(R, pad)
    if V["flag"]:
        return None
    Wa, Wb = int(min(2.0 * V["ha"], 2.0 * HALF_CAP)) + 1, int(min(2.0 * V["hb"], 2.0 * HALF_CAP)) + 1
    i0, i1, k2 = np.meshgrid(np.arange(PN), np.arange(PN), np.arange(PH), indexing="ij")
    i0, i1, k2 = i0.ravel(), i1.ravel(), k2.ravel()
    s0 = np.where(i0 <= PN // 2, i0, i0 - PN)
    s1 = np.where(i1 <= PN // 2, i1, i1 - PN)
    reach = (np.abs(s0) <= MP) & (np.abs(s1) <= MP) & (k2 <= MP)
    flat = (i0 * PN + i1) * PH + k2
    dp = float(pad)
    rows = []
    for sg in (0, 1):
        act = reach & ((sg == 0) | (k2 > 0))
        sign = -1.0 if sg else 1.0
        t = [sign * s0[act], sign * s1[act], sign * k2[act]]
        fl = flat[act]
        p0 = (R[0, 0] * t[0] + R[0, 1] * t[1]) + R[0, 2] * t[2]
        p1 = (R[1, 0] * t[0] + R[1, 1] * t[1]) + R[1, 2] * t[2]
        As = V["m00"] * p0 + V["m01"] * p1
        Bs = V["m01"] * p0 + V["m11"] * p1
        aF, bF = np.ceil(As - V["ha"]).astype(np.int64), np.ceil(Bs - V["hb"]).astype(np.int64)
        for ja in range(Wa):
            for jb in range(Wb):
                a, b = aF + ja, bF + jb
                ok = (b >= 0) & (a * a + b * b <= M * M)
                da, db = a.astype(np.float64), b.astype(np.float64)
                q = [dp * ((da * R[0, j]) + (db * R[1, j])) for j in range(3)]
                ok &= (np.abs(q[0]) < PN) & (np.abs(q[1]) < PN) & (np.abs(q[2]) < PN)
                c = [np.floor(x) for x in q]
                f = [x - y for x, y in zip(q, c)]
                g = [1.0 - x for x in f]
                d = [t[j] - c[j] for j in range(3)]
                for j in range(3):
                    ok &= (d[j] == 0.0) | (d[j] == 1.0)
                w = (np.where(d[0] == 1.0, f[0], g[0]) * np.where(d[1] == 1.0, f[1], g[1])) * np.where(d[2] == 1.0, f[2], g[2])
                rows.append((fl[ok], np.full(ok.sum(), sg), a[ok], b[ok], w[ok]))
    out = Taps()
    out.vox, out.neg, out.a, out.b, out.wt = (np.concatenate([r[i] for r in rows]) for i in range(5))
    out.neg = out.neg.astype(bool)
    return out


def tap_table(t):
    """the taps as rows (voxel, target, a, b, bits of wt), sorted: two enumerations agree iff their tables are equal"""
    order = np.lexsort((t.b, t.a, t.neg, t.vox))
    return np.stack([t.vox[order], t.neg[order].astype(np.int64), t.a[order], t.b[order],
                     t.wt[order].view(np.int64)], axis=1)


class Back:
    pass


def backproject_terms(Y, N, pad, Rs):
    """every forward tap of every view as a term of its voxel, in the kernel's order within a voxel: sorted by (voxel, view,
    target, a, b).  Returns the sorted arrays (vox, view, re, im, slack) with slack = 3 dq (|Re y| + |Im y|)."""
    Y = np.asarray(Y, dtype=np.complex128)
    H = N // 2 + 1
    cols = [[] for _ in range(7)]
    for v, R in enumerate(Rs):
        t = forward_taps(N, pad, R)
        y = Y[v][t.a % N, t.b]
        re = t.wt * y.real
        im = t.wt * np.where(t.neg, -y.imag, y.imag)
        for lst, x in zip(cols, (t.vox, np.full(len(t.vox), v), t.neg, t.a, t.b, re + 1j * im,
                                 3.0 * t.dq * (np.abs(y.real) + np.abs(y.imag)))):
            lst.append(x)
    vox, view, neg, a, b, term, slack = (np.concatenate(c) for c in cols)
    order = np.lexsort((b, a, neg, view, vox))
    assert H == Y.shape[-1]
    return vox[order], view[order], term[order], slack[order]


def backproject(terms, N, pad, nViews=None):
    """A of the first nViews views from backproject_terms: b.seq the terms added one after the other in the kernel's order,
    b.fsum with math.fsum, b.count the terms of a voxel, b.abs_re / b.abs_im the sums of |term| and b.slack of 3 dq |y|"""
    cv = conventions(N, pad)
    PN, PH = cv["PN"], cv["PH"]
    vox, view, term, slack = terms
    if nViews is not None:
        keep = view < nViews
        vox, term, slack = vox[keep], term[keep], slack[keep]
    V = PN * PN * PH
    out = Back()
    out.count = np.bincount(vox, minlength=V)
    start = np.concatenate([[0], np.cumsum(out.count)[:-1]])
    sr, si = np.zeros(V), np.zeros(V)
    has = np.nonzero(out.count)[0]
    for r in range(int(out.count.max()) if len(vox) else 0):
        has = has[out.count[has] > r]
        idx = start[has] + r
        sr[has] = sr[has] + term.real[idx]
        si[has] = si[has] + term.imag[idx]
    out.seq = (sr + 1j * si).reshape(PN, PN, PH)
    fr, fi = np.zeros(V), np.zeros(V)
    tr, ti = term.real.tolist(), term.imag.tolist()
    for s in np.nonzero(out.count)[0]:
        a, b = start[s], start[s] + out.count[s]
        fr[s] = math.fsum(tr[a:b])
        fi[s] = math.fsum(ti[a:b])
    out.fsum = (fr + 1j * fi).reshape(PN, PN, PH)
    out.abs_re = np.bincount(vox, weights=np.abs(term.real), minlength=V).reshape(PN, PN, PH)
    out.abs_im = np.bincount(vox, weights=np.abs(term.imag), minlength=V).reshape(PN, PN, PH)
    out.slack = np.bincount(vox, weights=slack, minlength=V).reshape(PN, PN, PH)
    out.count = out.count.reshape(PN, PN, PH)
    return out


def insert_bound(b):
    """(bound of the real parts, bound of the imaginary parts) of |device - b.fsum|"""
    return (b.count + C_TERM) * U * b.abs_re + b.slack, (b.count + C_TERM) * U * b.abs_im + b.slack


def fsum_bound(b):
    """|b.fsum - exact| per component: the roundings of a term alone (no summation error), and the coordinate slack"""
    return C_TERM * U * b.abs_re + b.slack, C_TERM * U * b.abs_im + b.slack


# ---- the passes back to the volume ----
def centre_phase(N, pad, centre):
    """phi[k] of the stored indices: twP[(o s) mod PN] e0 e1 e2, the factors multiplied in the library's order"""
    cv = conventions(N, pad)
    PN, PH, o = cv["PN"], cv["PH"], cv["o"]
    i = np.arange(PN)
    k = np.where(i <= PN // 2, i, i - PN)
    s = (k[:, None, None] + k[None, :, None] + np.arange(PH)[None, None, :]) % PN
    tw = twiddle_table(PN)
    c = np.zeros(3) if centre is None else np.asarray(centre, dtype=np.float64)
    e = []
    for d in range(3):
        kk = k if d < 2 else np.arange(PH)
        e.append(np.array([complex(1.0, 0.0) if c[d] == 0.0 else
                           complex(math.cos(2.0 * math.pi * (float(x) * c[d]) / float(PN)),
                                   math.sin(2.0 * math.pi * (float(x) * c[d]) / float(PN))) for x in kk]))
    return [tw[(o * s) % PN], e[0][:, None, None], e[1][None, :, None], e[2][None, None, :]]


def sinc2_table(N, pad):
    t = np.pi * (np.arange(N, dtype=np.float64) - (N + 1) // 2) / float(pad * N)
    s = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t))
    return s * s


def adjoint_volume(A, N, pad, centre=None, precorrect=False):
    """gvol [N, N, N] from A [PN, PN, PH]: A conj(phi), then gv[x] = sum_{stored k} Re(A_spec[k] twP[(k.x) mod PN])"""
    cv = conventions(N, pad)
    PN, PH = cv["PN"], cv["PH"]
    S = np.asarray(A, dtype=np.complex128)
    assert S.shape == (PN, PN, PH)
    for w in centre_phase(N, pad, centre):
        S = S * np.conj(w)
    tw = twiddle_table(PN)
    F = tw[(np.arange(PN)[:, None] * np.arange(N)[None, :]) % PN]      # [k, x]
    g = np.einsum("ijk,ix->xjk", S, F)
    g = np.einsum("xjk,jy->xyk", g, F)
    g = np.einsum("xyk,kz->xyz", g, F[:PH]).real
    if precorrect:
        s = sinc2_table(N, pad)
        g = g / ((s[:, None, None] * s[None, :, None]) * s[None, None, :])
    return g


def adjoint_bound(A, N, pad, precorrect=False):
    """|device - adjoint_volume| per voxel (both sides' roundings: twice the bound of one)"""
    cv = conventions(N, pad)
    S = np.abs(np.asarray(A).real).sum() + np.abs(np.asarray(A).imag).sum()
    b = 2.0 * 8.0 * (cv["PN"] + 16) * U * S * np.ones((N, N, N))
    if precorrect:
        s = sinc2_table(N, pad)
        b = b / ((s[:, None, None] * s[None, :, None]) * s[None, None, :]) * (1.0 + 8.0 * U)
    return b


def volume_spectrum(vol, N, pad, centre=None, precorrect=False):
    """C of a float64 volume in closed form (numpy double): the forward chain, for finite differences"""
    cv = conventions(N, pad)
    PN, PH = cv["PN"], cv["PH"]
    v = np.asarray(vol, dtype=np.float64)
    if precorrect:
        s = sinc2_table(N, pad)
        v = v / ((s[:, None, None] * s[None, :, None]) * s[None, None, :])
    tw = np.conj(twiddle_table(PN))
    F = tw[(np.arange(PN)[:, None] * np.arange(N)[None, :]) % PN]
    S = np.einsum("abx,kx->abk", v.astype(np.complex128), F[:PH])
    S = np.einsum("axk,jx->ajk", S, F)
    S = np.einsum("xjk,ix->ijk", S, F)
    for w in centre_phase(N, pad, centre):
        S = S * w
    return S


def slice_of(C, N, pad, R, shiftX=0, shiftY=0):
    """the slice [N, H] of C under R through forward_taps (terms added per coefficient in tap order), de-centred"""
    t = forward_taps(N, pad, R)
    H = N // 2 + 1
    PN, PH = pad * N, pad * N // 2 + 1
    v = np.asarray(C).reshape(-1)[t.vox]
    v = np.where(t.neg, np.conj(v), v)
    out = np.zeros(N * H, dtype=np.complex128)
    np.add.at(out, (t.a % N) * H + t.b, t.wt * v)
    assert C.shape == (PN, PN, PH)
    a, b = stored(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    return out.reshape(N, H) * twiddle_table(N)[twiddle_index(A, B, N, shiftX, shiftY)]


# ---- log P of one request as a function of the float volume (the direction test, and its check against the oracle) ----
class LogPChain:
    """One request (orientation quat, CTF kernel K [N, H, 2] float32 with its parameters ctf3, particle spectrum F [N, H, 2]
    float32 with its sums, shift (x, y)) on a volume model (N, pad, centre, the handle's shifts, precorrection on).  The
    slices come from slice_reference (sequential sums) on the double spectrum of the float volume.
      float_point / float_logp   the slice rounded to float2 into the oracle's convolution and calc_logpro: the CPU float chain
      point64 / logp64           the float64 closed form of gradient_reference on the double slice (CTF priors left out)
      gradient64                 its gradient with respect to the volume through this module's adjoint chain"""

    def __init__(self, N, pad, centre, shift, quat, K, ctf3, F, sumRef, sumsqRef, x, y, opd):
        self.N, self.pad, self.centre, self.shift, self.quat = N, pad, centre, tuple(shift), np.asarray(quat, dtype=np.float32)
        self.K, self.ctf3, self.F = np.ascontiguousarray(K, dtype=np.float32), ctf3, np.ascontiguousarray(F, dtype=np.float32)
        self.sumRef, self.sumsqRef, self.x, self.y, self.opd = float(sumRef), float(sumsqRef), int(x), int(y), opd

    @staticmethod
    def _c(a):
        return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)

    def slice64(self, vol):
        import slice_reference as sr
        v = np.asarray(vol, dtype=np.float32).astype(np.float64)
        C = volume_spectrum(v, self.N, self.pad, self.centre, precorrect=True)
        return sr.slice_sequential(sr.slice_terms(C, self.N, self.pad, self.quat, True), self.N, *self.shift)

    def float_point(self, vol):
        """(q, cc): the oracle's parameters {amp, pha, env, sumC, sumsquareC} and its float cc at the request's shift"""
        import oracle as orc
        import window_reference as wr
        s = self.slice64(vol)
        proj = np.ascontiguousarray(np.stack([s.real, s.imag], axis=-1).astype(np.float32))
        conv, sC, ssC = orc.convolve(proj, self.K)
        q = dict(amp=self.ctf3[0], pha=self.ctf3[1], env=self.ctf3[2], sumC=sC, sumsquareC=ssC)
        Sg, _ = wr.s_map(conv, self.F)
        return q, wr.cc_of(Sg[(-self.x) % self.N, (-self.y) % self.N], self.N)

    def float_logp(self, vol):
        import window_reference as wr
        q, cc = self.float_point(vol)
        return float(wr.logpro(self.opd, q, cc, self.sumRef, self.sumsqRef))

    def point64(self, vol):
        import gradient_reference as gr
        conv = self.slice64(vol) * np.conj(self._c(self.K))
        return conv, gr.sums(conv, self._c(self.F), self.x, self.y) + (self.sumRef, self.sumsqRef, float(self.N * self.N))

    def logp64(self, vol):
        import gradient_reference as gr
        return gr.logp(*self.point64(vol)[1])

    def gradient64(self, vol):
        import gradient_reference as gr
        conv, point = self.point64(vol)
        a, b, g = gr.coefficients(*point)
        GP = gr.gradient_spectrum(a, b, g, conv, self._c(self.F), self._c(self.K), self.x, self.y)
        Y = prepare_y(GP[None], self.N, None, *self.shift, full=True)
        A = backproject(backproject_terms(Y, self.N, self.pad, [matrix(self.quat)]), self.N, self.pad).fsum
        return adjoint_volume(A, self.N, self.pad, self.centre, True)
