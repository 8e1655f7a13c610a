"""The 3D density the aligned view sums support (Engine.reconstruct; include/bioem_hip.h): what the host does
with the device's volumes -- the Fourier shell correlation of two half-set reconstructions, the resolution read off it,
the MRC volume a run reads back with --ReadModelMRC, and the text file of the shells.

The text file: after the HEADER:: NOTATION bar, one notation line and the bar again, one line per shell s >= 0

 SHELL s resolution weight FSC cross powA powB

(resolution = N pixelSize / s in Angstrom, 0 for shell 0; weight = coefficients of the full spectrum in the shell; FSC =
cross / sqrt(powA powB), 0 where the product is 0) and one line

 DATASET views particles tau res05 res0143

(res05 / res0143: the resolution of the first shell s >= 1 with FSC below 0.5 / 0.143, -1 if none), floating values with
16 significant digits; the CLI's --Reconstruct writes the same layout (bioem_amd/host/reconstruct.cpp).

The MRC volume: --ReadModelMRC places file voxel e (from 0, first file axis slowest) at (e + 1 - N / 2) pixelSize on each
axis; the reconstruction has its origin at voxel o = (N + 1) / 2.  write_mrc therefore stores file[e] = vol[(e + 1) mod N]
on every axis, a cyclic shift by one voxel: for even N a read-back point sits exactly where the reconstruction has it,
for odd N half a pixel beyond it on every axis (N / 2 is not a whole number there)."""
import struct

import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"
NOTATION = (" SHELL: shell resolution[A] weight FSC cross powHalf1 powHalf2   DATASET: views particles tau "
            "resolution[A](FSC<0.5) resolution[A](FSC<0.143)")
SHELL_DTYPE = np.dtype([("shell", "<i4"), ("resolution", "<f8"), ("weight", "<f8"), ("FSC", "<f8"), ("cross", "<f8"),
                        ("powA", "<f8"), ("powB", "<f8")])
DATASET_DTYPE = np.dtype([("views", "<i8"), ("particles", "<i8"), ("tau", "<f8"), ("res05", "<f8"), ("res0143", "<f8")])


def shell_index(N):
    """(shell int [N, N, H], Hermitian weight float [N, N, H]) of the stored half spectrum: the rounded |kappa| of the
    centred frequency, and 2 for a coefficient whose conjugate partner is not stored (0 < k2, 2 k2 != N), else 1, so
    that the weights add up to N^3"""
    H = N // 2 + 1
    i = np.arange(N)
    k = np.where(i <= N // 2, i, i - N).astype(np.float64)
    k2 = np.arange(H, dtype=np.float64)
    r = np.sqrt(k[:, None, None] ** 2 + k[None, :, None] ** 2 + k2[None, None, :] ** 2)
    w = np.where((np.arange(H) > 0) & (2 * np.arange(H) != N), 2.0, 1.0)
    return np.floor(r + 0.5).astype(np.int64), np.broadcast_to(w[None, None, :], (N, N, H)).copy()


def shell_sums(specA, specB):
    """per shell (weight, cross = sum w Re(A conj(B)), powA = sum w |A|^2, powB = sum w |B|^2) of two spectra [N, N, H]"""
    A = np.asarray(specA, dtype=np.complex128)
    B = np.asarray(specB, dtype=np.complex128)
    N = A.shape[0]
    assert A.shape == (N, N, N // 2 + 1) and B.shape == A.shape
    s, w = shell_index(N)
    n = int(s.max()) + 1
    s, w = s.ravel(), w.ravel()
    a, b = A.ravel(), B.ravel()
    fold = lambda x: np.bincount(s, weights=w * x, minlength=n)
    return fold(np.ones(len(s))), fold(a.real * b.real + a.imag * b.imag), fold(a.real ** 2 + a.imag ** 2), \
        fold(b.real ** 2 + b.imag ** 2)


def fsc(cross, powA, powB):
    d = np.asarray(powA, dtype=np.float64) * np.asarray(powB, dtype=np.float64)
    return np.where(d > 0, np.asarray(cross, dtype=np.float64) / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)


def derive(cross, powA, powB, N, pixel_size):
    """(FSC [nShells], resolution [nShells], res05, res0143) as the writer prints them"""
    f = fsc(cross, powA, powB)
    size = float(N) * float(np.float32(pixel_size))
    s = np.arange(len(f))
    res = np.where(s > 0, size / np.maximum(s, 1), 0.0)
    out = []
    for thr in (0.5, 0.143):
        below = f[1:] < thr
        out.append(float(res[below.argmax() + 1]) if below.any() else -1.0)
    return f, res, out[0], out[1]


def half_weights(n):
    """(even, odd): float64 [n] weights that keep the particles 0, 2, ... and 1, 3, ..."""
    p = np.arange(int(n))
    return (p % 2 == 0).astype(np.float64), (p % 2 == 1).astype(np.float64)


def write_mrc(path, vol, pixel_size=1.0):
    """a volume [N, N, N] (origin at voxel (o, o, o), axes x, y, z) as the mode-2 MRC file --ReadModelMRC reads back"""
    vol = np.asarray(vol, dtype=np.float32)
    N = vol.shape[0]
    assert vol.shape == (N, N, N)
    hdr = np.zeros(256, dtype="<i4")
    hdr[0:4] = [N, N, N, 2]
    hdr[7:10] = [N, N, N]
    raw = hdr.tobytes()
    cell = float(N) * float(pixel_size)
    raw = raw[:40] + struct.pack("<6f", cell, cell, cell, 90., 90., 90.) + raw[64:]
    label = ("bioem_amd reconstruction: file[e] = vol[(e + 1) mod N] per axis, origin voxel %d" % ((N + 1) // 2)).encode()
    raw = raw[:220] + struct.pack("<i", 1) + label.ljust(80)[:80] + raw[304:]   # NLABL and the first label
    assert len(raw) == 1024
    with open(path, "wb") as f:
        f.write(raw + np.ascontiguousarray(np.roll(vol, (-1, -1, -1), axis=(0, 1, 2)), dtype="<f4").tobytes())


def read_mrc(path):
    """the volume write_mrc stored, the shift undone: float32 [N, N, N]"""
    with open(path, "rb") as f:
        raw = f.read()
    nc, nr, ns, mode = struct.unpack("<4i", raw[:16])
    nsymbt = struct.unpack("<i", raw[92:96])[0]
    if mode != 2 or not (nc == nr == ns) or len(raw) < 1024 + nsymbt + 4 * nc * nr * ns:
        raise ValueError("%s: not a cubic mode-2 MRC volume" % path)
    data = np.frombuffer(raw, dtype="<f4", count=nc ** 3, offset=1024 + nsymbt).reshape(nc, nc, nc)
    return np.roll(data, (1, 1, 1), axis=(0, 1, 2)).astype(np.float32)


def write(path, sums, N, pixel_size, views, particles, tau):
    """the text file of the shell sums (weight, cross, powA, powB) of shell_sums"""
    weight, cross, pa, pb = (np.asarray(x, dtype=np.float64) for x in sums)
    f, res, r05, r0143 = derive(cross, pa, pb, N, pixel_size)
    with open(path, "w") as out:
        out.write(BAR + "\n" + NOTATION + "\n" + BAR + "\n")
        for s in range(len(f)):
            out.write("SHELL %d %.15e %.15e %.15e %.15e %.15e %.15e\n" % (s, res[s], weight[s], f[s], cross[s], pa[s], pb[s]))
        out.write("DATASET %d %d %.15e %.15e %.15e\n" % (int(views), int(particles), float(tau), r05, r0143))


def parse(path):
    """Returns (shells [nShells] of SHELL_DTYPE, dataset of DATASET_DTYPE).  Raises ValueError for a file that is not of
    the layout above."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    shells, data = [], []
    for ln in lines[3:]:
        if not ln.strip():
            continue
        t = ln.split()
        if t[0].startswith("SOFT"):   # the lines --ReconstructSoft adds (bioem_amd/soft_views.py)
            continue
        if t[0] == "SHELL" and len(t) == 8:
            shells.append((int(t[1]),) + tuple(float(x) for x in t[2:]))
        elif t[0] == "DATASET" and len(t) == 6:
            data.append((int(t[1]), int(t[2])) + tuple(float(x) for x in t[3:]))
        else:
            raise ValueError("%s: malformed line %r" % (path, ln))
    shells = np.array(shells, dtype=SHELL_DTYPE)
    if len(data) != 1 or (shells["shell"] != np.arange(len(shells))).any():
        raise ValueError("%s: shells out of order or not exactly one DATASET line" % path)
    return shells, np.array(data, dtype=DATASET_DTYPE)[0]
