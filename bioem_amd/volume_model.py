"""A volume as the model (Engine.upload_model_volume / upload_model_spectrum; include/bioem_hip.h): what the
host states about it in numpy -- the centre of mass the upload can remove, the padded spectrum the upload forms, the
centred spectrum the handle keeps, and the way from a reconstruction back into a run.

Conventions: N, o = (N + 1) // 2 the origin voxel, P the padding, PN = P N, PH = PN // 2 + 1; a stored index
i <= PN // 2 of axes 0 and 1 stands for the frequency i, a larger one for i - PN; axis 2 is the half axis."""
import numpy as np


def origin(N):
    return (int(N) + 1) // 2


def centre_of_mass(vol):
    """the centre of mass of vol [N, N, N] in voxels relative to the origin voxel (o, o, o), float64 [3], summed in double"""
    v = np.asarray(vol, dtype=np.float64)
    N = v.shape[0]
    assert v.shape == (N, N, N)
    total = v.sum()
    if not total != 0.0:
        raise ValueError("the volume's total density is 0: no centre of mass")
    x = np.arange(N, dtype=np.float64) - origin(N)
    return np.array([(v.sum(axis=(1, 2)) * x).sum(), (v.sum(axis=(0, 2)) * x).sum(), (v.sum(axis=(0, 1)) * x).sum()]) / total


def sinc2_table(N, pad):
    """sinc^2(pi (x - o) / PN) for x = 0 ... N - 1: the transform of the trilinear kernel on the padded grid, as the upload
    makes it on the host"""
    t = np.pi * (np.arange(N, dtype=np.float64) - origin(N)) / float(pad * N)
    s = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t))
    return s * s


def precorrected(vol, pad):
    """vol / prod_d sinc^2(pi (x_d - o) / PN) in double, the products in the upload's order"""
    v = np.asarray(vol, dtype=np.float32).astype(np.float64)
    s = sinc2_table(v.shape[0], pad)
    return v / ((s[:, None, None] * s[None, :, None]) * s[None, None, :])


def twiddles(PN):
    """exp(+2 pi i j / PN), j = 0 ... PN - 1, from the reduced index as every table of the library is built"""
    ang = 2.0 * np.pi * np.arange(PN, dtype=np.float64) / float(PN)
    return np.cos(ang) + 1j * np.sin(ang)


def pad_spectrum(vol, pad=2, precorrect=True):
    """spec[k] = sum_x vol[x] exp(-2 pi i k.x / PN) over the N^3 box in the first octant of the PN^3 box, complex128 [PN,
    PN, PH]: what upload_model_volume forms before it centres it, as three passes of N-term sums (axis 2, 1, 0) with the
    twiddle index (k x) mod PN reduced in integers; precorrect as there"""
    assert pad in (1, 2)
    v = precorrected(vol, pad) if precorrect else np.asarray(vol, dtype=np.float32).astype(np.float64)
    N = v.shape[0]
    assert v.shape == (N, N, N)
    PN = pad * N
    PH = PN // 2 + 1
    tw = np.conj(twiddles(PN))
    F = tw[(np.arange(PN)[:, None] * np.arange(N)[None, :]) % PN]     # [k, x]
    s = np.einsum("abx,kx->abk", v.astype(np.complex128), F[:PH])     # axis 2
    s = np.einsum("axk,jx->ajk", s, F)                                # axis 1
    return np.einsum("xjk,ix->ijk", s, F)                             # axis 0


def centre_tables(PN, centre):
    """e_d[i] = exp(+2 pi i k centre_d / PN) for the stored index i of an axis (k = i, or i - PN beyond PN // 2), [3, PN]"""
    i = np.arange(PN)
    k = np.where(i <= PN // 2, i, i - PN).astype(np.float64)
    c = np.zeros(3) if centre is None else np.asarray(centre, dtype=np.float64)
    out = np.ones((3, PN), dtype=np.complex128)
    for d in range(3):
        if c[d] != 0.0:
            ang = 2.0 * np.pi * (k * c[d]) / float(PN)
            out[d] = np.cos(ang) + 1j * np.sin(ang)
    return out


def centred_spectrum(spec, N, pad, centre=None):
    """C(k') = spec[k' mod PN] twP[(o (k'0 + k'1 + k'2)) mod PN] e0 e1 e2, complex128 [PN, PN, PH]: the spectrum about the
    origin voxel of the density moved by -centre, what the handle keeps; the products in the library's order"""
    spec = np.asarray(spec, dtype=np.complex128)
    PN = pad * N
    PH = PN // 2 + 1
    assert spec.shape == (PN, PN, PH)
    i = np.arange(PN)
    k = np.where(i <= PN // 2, i, i - PN)
    s = (k[:, None, None] + k[None, :, None] + np.arange(PH)[None, None, :]) % PN
    e = centre_tables(PN, centre)
    C = spec * twiddles(PN)[(origin(N) * s) % PN]
    C = C * e[0][:, None, None]
    C = C * e[1][None, :, None]
    return C * e[2][None, None, :PH]


def from_reconstruction(result):
    """(spec, pad) for Engine.upload_model_spectrum from the dict of Engine.reconstruct(..., want_spec=True): the estimate
    V^ itself, un-centred [N, N, H], at pad = 1"""
    if "spec" not in result:
        raise ValueError("the reconstruction holds no spectrum: call Engine.reconstruct(..., want_spec=True)")
    return np.ascontiguousarray(result["spec"], dtype=np.complex128), 1
