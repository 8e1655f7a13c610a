"""CPU tests of the reference of the volume gradient (tests/volume_gradient_reference.py; vgrad_kernels.hpp): the
gather enumeration of k_vgrad_insert against the forward's tap set, the adjoint identity, the chain back to the volume
against finite differences of the double closed form, the scaling of Y against the c2r, and the plumbing."""
import math
import os
import re

import numpy as np
import pytest

import volume_gradient_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z45 = np.array([0, 0, math.sin(math.pi / 8), math.cos(math.pi / 8)])


def quaternions(seed, n, length):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    q = q / np.linalg.norm(q, axis=1)[:, None]
    q[0] = Z45
    return (length * q).astype(np.float32)


def dot(x, y):
    """sum Re(conj(x) y), exactly rounded"""
    x, y = np.asarray(x).ravel(), np.asarray(y).ravel()
    return math.fsum((x.real * y.real).tolist() + (x.imag * y.imag).tolist())


@pytest.mark.parametrize("N", [8, 9])
@pytest.mark.parametrize("pad", [1, 2])
@pytest.mark.parametrize("length", [1.0, 1.07, 0.85])
def test_gather_enumeration_equals_the_forward_tap_set(N, pad, length):
    """every tap of the forward is found from its voxel's side with the forward's weight bits, and nothing else is"""
    total = 0
    for q in quaternions(7 * N + pad, 6, length):
        R = vr.matrix(q)
        f, g = vr.forward_taps(N, pad, R), vr.gather_taps(N, pad, R)
        assert g is not None
        tf, tg = vr.tap_table(f), vr.tap_table(g)
        assert tf.shape == tg.shape and np.array_equal(tf, tg)
        # a coefficient reaches a voxel under a target at most once: the kernel's order within a voxel is total
        assert len(np.unique(tf[:, :4], axis=0)) == len(tf)
        total += len(tf)
    assert total > 0


def test_half_widths_and_refusals():
    """sqrt(3) sqrt((G^-1)_dd) / P against numpy's inverse; beyond the cap and rank-deficient matrices are flagged"""
    for pad in (1, 2):
        for length in (1.0, 1.07, 0.85):
            for q in quaternions(9, 50, length):
                R = vr.matrix(q)
                V = vr.view_parameters(R, pad)
                Gi = np.linalg.inv(R[:2] @ R[:2].T)
                assert V["flag"] == 0
                for key, d in (("ha", 0), ("hb", 1)):
                    assert abs(V[key] - vr.SQRT3 * math.sqrt(Gi[d, d]) / pad) < 1e-5
                if length == 1.0:
                    assert abs(V["ha"] - vr.SQRT3 / pad) < 1e-5
    short = vr.matrix(np.array([0.6, 0, 0, 0], dtype=np.float32))     # diag(1, 0.28, 0.28): half-width sqrt(3) / 0.28 / P
    assert vr.view_parameters(short, 1)["flag"] == 2
    assert vr.gather_taps(8, 1, short) is None
    assert vr.view_parameters(short, 2)["flag"] == 0
    assert vr.view_parameters(np.zeros((3, 3)), 1)["flag"] == 1
    R = np.eye(3)
    R[1] = R[0]
    assert vr.view_parameters(R, 1)["flag"] == 1
    R[1, 0] = np.nan
    assert vr.view_parameters(R, 2)["flag"] == 1
    # the documented candidate counts of a rotation: 4 per axis at pad 1, 2 at pad 2
    for pad, count in ((1, 4), (2, 2)):
        V = vr.view_parameters(np.eye(3), pad)
        assert int(2.0 * V["ha"]) + 1 == count


@pytest.mark.parametrize("N,pad", [(8, 1), (9, 2)])
def test_adjoint_identity(N, pad):
    """<Gamma, slice(C)> = <A, C> within the rounding of the terms"""
    rng = np.random.default_rng(N + pad)
    PN, PH, H = pad * N, pad * N // 2 + 1, N // 2 + 1
    C = rng.standard_normal((PN, PN, PH)) + 1j * rng.standard_normal((PN, PN, PH))
    qs = quaternions(3, 5, 1.0)
    qs[1] = (1.07 * Z45).astype(np.float32)
    Rs = [vr.matrix(q) for q in qs]
    G = rng.standard_normal((5, N, H)) + 1j * rng.standard_normal((5, N, H))
    w = rng.uniform(-2, 2, 5)
    Y = vr.prepare_y(G, N, w, 3, -2, full=False)
    b = vr.backproject(vr.backproject_terms(Y, N, pad, Rs), N, pad)
    # the slice side from slice_reference (its own statement of the forward, math.fsum over a coefficient's eight terms)
    import slice_reference as sr
    lhs, tol = [], 0.0
    for v in range(5):
        r = sr.slice_terms(C, N, pad, qs[v], True)
        lhs.append(w[v] * dot(G[v], sr.slice_fsum(r, N, 3, -2)))
        tol += abs(w[v]) * float(((np.abs(G[v].real) + np.abs(G[v].imag)) * sr.slice_bound(r)).sum())
        assert np.abs(vr.slice_of(C, N, pad, Rs[v], 3, -2) - sr.slice_sequential(r, N, 3, -2)).max() <= 64 * vr.U * np.abs(C).max()
    lhs = math.fsum(lhs)
    rhs = dot(b.fsum, C)
    br, bi = vr.fsum_bound(b)
    tol += float((br * np.abs(C.real) + bi * np.abs(C.imag)).sum()) + 64 * vr.U * float(
        (b.abs_re * np.abs(C.real) + b.abs_im * np.abs(C.imag)).sum())
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)
    assert abs(lhs) > 1e6 * tol


def test_chain_against_finite_differences():
    """N = 8, pad 2, centre != 0, shift (3, -2), precorrection: a central difference of sum Re(conj Gamma slice) over float64
    volumes against <gvol, d>.  The form is linear in the volume: the difference is exact up to rounding."""
    N, pad, centre, sx, sy = 8, 2, np.array([0.3, -0.7, 1.1]), 3, -2
    rng = np.random.default_rng(5)
    H = N // 2 + 1
    vol, d = rng.uniform(0.1, 1.0, (N, N, N)), rng.standard_normal((N, N, N))
    qs = quaternions(11, 4, 1.0)
    Rs = [vr.matrix(q) for q in qs]
    G = rng.standard_normal((4, N, H)) + 1j * rng.standard_normal((4, N, H))
    Y = vr.prepare_y(G, N, None, sx, sy, full=False)
    masked = np.where(np.abs(Y) > 0, G, 0)

    def L(v):
        C = vr.volume_spectrum(v, N, pad, centre, precorrect=True)
        return math.fsum(dot(masked[i], vr.slice_of(C, N, pad, Rs[i], sx, sy)) for i in range(4))

    b = vr.backproject(vr.backproject_terms(Y, N, pad, Rs), N, pad)
    gvol = vr.adjoint_volume(b.fsum, N, pad, centre, precorrect=True)
    h = 0.25
    fd = (L(vol + h * d) - L(vol - h * d)) / (2 * h)
    got = float((gvol * d).sum())
    scale = float((np.abs(gvol) * np.abs(d)).sum())
    assert abs(fd - got) <= 1e-10 * scale, (fd, got)
    assert abs(got) > 1e-3 * scale


@pytest.mark.parametrize("N", [8, 9])
def test_scale_of_y_against_the_c2r(N):
    """sum_x c2r(G^)[x] p[x] / N^2 = sum_stored (w_b / N^2) Re(conj(Gamma) p^) for an image p band-limited to the disc:
    the symmetrisation, w_b and 1 / N^2 of the full Y state the pixel-space gradient G_P = c2r(G^_P) / N^2"""
    rng = np.random.default_rng(N)
    H, M = N // 2 + 1, (N - 1) // 2
    a, b = vr.stored(N)
    A, B = np.meshgrid(a, b, indexing="ij")
    disc = A * A + B * B <= M * M
    p = np.fft.irfft2(np.where(disc, np.fft.rfft2(rng.standard_normal((N, N))), 0), s=(N, N))
    P = np.fft.rfft2(p)
    G = rng.standard_normal((N, H)) + 1j * rng.standard_normal((N, H))
    lhs = float((np.fft.irfft2(G, s=(N, N)) * p).sum())          # (irfft2 divides by N^2 and keeps the Hermitian part)
    Y = vr.prepare_y(G[None], N, np.array([1.0]), 0, 0, full=True)[0]
    tw = vr.twiddle_table(N)[vr.twiddle_index(A, B, N, 0, 0)]
    rhs = dot(Y * tw, P)                                          # (Y carries conj(tw): undone here)
    assert abs(lhs - rhs) <= 1e-12 * float(np.abs(G).sum() * np.abs(p).max())


def test_exports_and_header_declarations():
    from bioem_amd import engine
    names = ["bioem_hip_volume_gradient", "bioem_hip_debug_volume_backproject", "bioem_hip_debug_volume_adjoint"]
    with open(os.path.join(ROOT, "include", "bioem_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in engine.EXPORTS
        assert re.search(r"^int %s\(bioem_hip_handle h," % n, header, re.M)
    for m in ("volume_gradient", "best_match_volume_gradient", "debug_volume_backproject", "debug_volume_adjoint"):
        assert callable(getattr(engine.Engine, m))
    with open(os.path.join(ROOT, "bioem_amd", "csrc", "vgrad_kernels.hpp")) as f:
        src = f.read()
    assert "#define BIOEM_VGRAD_HALF_CAP %.1f" % vr.HALF_CAP in src


def test_writer_and_parser_round_trip(tmp_path):
    from bioem_amd import reconstruct, volume_gradient as vg
    N = 9
    rng = np.random.default_rng(1)
    g, vol = rng.standard_normal((N, N, N)), rng.uniform(0, 1, (N, N, N)).astype(np.float32)
    d = vg.derive(g, vol)
    assert abs(d["vol_dot_g"] - float((vol.astype(np.float64) * g).sum())) <= 1e-12
    assert abs(d["step"].sum()) <= 1e-9 and d["shells"]["voxels"].sum() == N ** 3
    assert abs(d["shells"]["vol_dot_g"].sum() - d["vol_dot_g"]) <= 1e-12 and abs(d["shells"]["power"].sum() - d["norm"] ** 2) <= 1e-9
    # the shell of a voxel by a loop
    s = vg.shell_index(N)
    o = (N + 1) // 2
    for x in ((0, 0, 0), (o, o, o), (8, 2, 5)):
        assert s[x] == int(math.floor(math.sqrt(sum((v - o) ** 2 for v in x)) + 0.5))
    path = str(tmp_path / "vg.txt")
    vg.write(path, g, vol, 1.5, requests=7, sumw=6.5, nonfinite=1)
    back = vg.parse(path)
    assert back["shells"].tobytes() == d["shells"].tobytes()
    assert back["dataset"] == {"vol_dot_g": d["vol_dot_g"], "norm": d["norm"], "requests": 7, "sumw": 6.5, "nonfinite": 1}
    assert np.array_equal(reconstruct.read_mrc(path + ".mrc"), g.astype(np.float32))
    (tmp_path / "bad.txt").write_text("SHELL 0 1 0 0 0\n")
    with pytest.raises(ValueError, match="no DATASET"):
        vg.parse(str(tmp_path / "bad.txt"))
    (tmp_path / "bad2.txt").write_text("SHELL 0 1 0 0\nDATASET 0 0 0 0 0\n")
    with pytest.raises(ValueError, match="bad SHELL"):
        vg.parse(str(tmp_path / "bad2.txt"))


def test_cli_names_the_option_and_its_refusals(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,  # noqa: E731
                                      text=True, timeout=60)
    assert "--VolumeGradient" in run(["--help"]).stdout
    r = run(["--Modelfile", "m.mrc", "--VolumeGradient"])
    assert "requires an argument" in r.stdout and "Running" not in r.stdout
    r = run(["--Modelfile", "m.txt", "--Particlesfile", "p.txt", "--Inputfile", "i.txt", "--VolumeGradient", "vg"])
    assert r.returncode != 0 and "--VolumeGradient needs --ModelVolume" in r.stdout
    r = run(["--Modelfile", "m.mrc", "--Particlesfile", "p.txt", "--Inputfile", "i.txt", "--ModelVolume", "--ModelGradient", "g"])
    assert r.returncode != 0 and "--ModelVolume is not valid with --ModelGradient (the gradient is per model point; a volume " \
        "has none)" in r.stdout and "--VolumeGradient" in r.stdout
    from test_best_maps_host import QUAT_CTF
    (tmp_path / "best.txt").write_text(QUAT_CTF)
    r = run(["--Modelfile", "m.mrc", "--ModelVolume", "--PrintBestCalMap", "best.txt", "--VolumeGradient", "vg"])
    assert r.returncode != 0 and "--PrintBestCalMap" in r.stdout
    assert not (tmp_path / "vg").exists() and not (tmp_path / "vg.mrc").exists()


def test_logp_of_the_reference_against_the_oracle():
    """the chains of the direction test (volume_gradient_reference.LogPChain) on the CPU, as test_model_gradient_host.py does
    for points: slices of a volume from the reference go into the oracle's convolution and calc_logpro; the closed form at
    the oracle's linearisation point is calc_logpro less the CTF priors, within window_reference's bound for that comparison
    plus the float evaluation of the logarithms' arguments (8 roundings of 2^-24 on the magnitudes of their terms).  The
    float64 chain on the double slice differs from it by the float roundings of the linearisation point: the slice and
    the product with the kernel 3 2^-24 per coefficient, the float sum of sumsquareC (M + 9) 2^-24, cc 5 2^-24
    on the sum of the magnitudes of its terms, carried by |a|, |b|, |g| and doubled for the curvature."""
    import gradient_reference as gr
    import projection_reference as pr
    import window_reference as wr
    from golden_util import load_case, oracle_setup
    from test_model_gradient_host import ctf_prior
    S = oracle_setup(load_case("g3_n32_trace"))
    N, pad, centre, shift = S.N, 2, np.array([0.3, -0.2, 0.1]), (1, -1)
    Nt, M = float(N * N), N * (N // 2 + 1)
    rng = np.random.default_rng(12)
    x = np.arange(N) - (N + 1) // 2
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    vol = (rng.uniform(0.1, 1.0, (N, N, N)) * (r2 <= (N / 6.0) ** 2)).astype(np.float32)
    quats = pr.unit_quaternions(rng, 3)
    f24 = 2.0 ** -24
    for p in range(min(3, S.nMaps)):
        c = p % S.nCTF
        ch = vr.LogPChain(N, pad, centre, shift, quats[p], S.refCTF[c], S.ctfParam[c], S.refFFT[p], S.sumRef[p], S.sumsqRef[p],
                          (-2, 0, 3)[p], (1, -3, 0)[p], S.pd)
        q, cc = ch.float_point(vol)
        want = float(wr.logpro(S.pd, q, cc, S.sumRef[p], S.sumsqRef[p])) + ctf_prior(S.pd, q)
        assert abs(ch.float_logp(vol) + ctf_prior(S.pd, q) - want) == 0.0
        fe = float(wr.firstele(S.pd, q, cc, S.sumRef[p], S.sumsqRef[p]))
        bound = float(wr.logp_bound(S.pd, q, fe, N))
        point = [float(v) for v in (q["sumC"], q["sumsquareC"], cc, S.sumRef[p], S.sumsqRef[p])]
        s, ssq, c_, sr_, ssr = point
        F_, fe64 = gr.forlog(*point, Nt)
        assert F_ > 0 and fe64 > 0
        mag_fe = Nt * (abs(ssr * ssq) + c_ * c_) + abs(2 * sr_ * s * c_) + abs(ssr * s * s) + abs(sr_ * sr_ * ssq)
        mag_F = abs(ssq * Nt) + s * s
        extra = 8 * f24 * (abs(3 - Nt) / 2 * mag_fe / abs(fe64) + abs(Nt / 2 - 2) * mag_F / abs(F_))
        got = gr.logp(*point, Nt)
        assert abs(got - want) <= bound + extra, (p, got, want, bound, extra)
        # the float64 chain of the direction test against the same closed form at the float point
        conv, p64 = ch.point64(vol)
        a, b, g = gr.coefficients(*p64)
        Fc = S.refFFT[p][..., 0].astype(np.float64) + 1j * S.refFFT[p][..., 1].astype(np.float64)
        acc = float((np.abs(conv * np.conj(Fc)) * wr.weights(N)[None, :]).sum()) / Nt
        drift = 2.0 * f24 * (abs(a) * 3 * abs(p64[0]) + abs(b) * (M + 9) * abs(p64[1]) + abs(g) * 5 * acc)
        l64 = ch.logp64(vol)
        assert abs(l64 - got) <= drift, (p, l64, got, drift)
        print("particle %d: closed form - oracle = %.3g (bound %.3g), float64 chain - closed form = %.3g (bound %.3g)" % (
            p, got - want, bound + extra, l64 - got, drift))
