"""ctypes binding of the C++ host layer's C entry points (bioem_amd/host/capi.cpp, libbioem_host.so):
the one-off precompute the reference does on the host before the hot loop."""
import ctypes as C
import os

import numpy as np

from .engine import POINT_DTYPE, ParamDevice, load_library

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def load_host_library():
    global _lib
    if _lib is None:
        load_library()  # libbioem_hip.so first (dependency)
        path = os.path.join(HERE, "lib", "libbioem_host.so")
        if not os.path.exists(path):
            raise RuntimeError("host layer not built: %s missing (make -C bioem_amd/csrc host)" % path)
        L = C.CDLL(path)
        ci, cf, vp = C.c_int, C.c_float, C.c_void_p
        L.bioem_host_ctf_kernels.argtypes = [ci, cf, cf, cf, ci, cf, cf, ci, cf, cf, ci, vp, vp, vp]
        L.bioem_host_ctf_kernels.restype = ci
        L.bioem_host_volume_element.argtypes = [cf, ci, ci, cf, ci, cf, cf, cf, cf, cf]
        L.bioem_host_volume_element.restype = cf
        L.bioem_host_center_model.argtypes = [vp, ci]
        L.bioem_host_center_model.restype = cf
        _lib = L
    return _lib


def ctf_kernels(N, pixelSize, amp, phase, env):
    """amp/phase/env = (start, end, n) in the reference's internal units (phase = defocus*2*pi*1e4*lambda).
    Returns refCTF [nCTF,N,H,2], ctfParam [nCTF,3], steps[3]."""
    L = load_host_library()
    n = amp[2] * phase[2] * env[2]
    H = N // 2 + 1
    ref = np.zeros((n, N, H, 2), dtype=np.float32)
    par = np.zeros((n, 3), dtype=np.float32)
    steps = np.zeros(3, dtype=np.float32)
    got = L.bioem_host_ctf_kernels(N, pixelSize, amp[0], amp[1], amp[2], phase[0], phase[1], phase[2], env[0], env[1],
                                   env[2], ref.ctypes.data, par.ctypes.data, steps.ctypes.data)
    assert got == n
    return ref, par, steps


def psf_kernels(N, pixelSize, amp, phase, env, device=0):
    """ctf_kernels in PSF mode: the real-space kernels transformed on `device`, as the CLI's set-up makes them"""
    L = load_host_library()
    ci, cf, vp = C.c_int, C.c_float, C.c_void_p
    L.bioem_host_psf_kernels.argtypes = [ci, cf, cf, cf, ci, cf, cf, ci, cf, cf, ci, vp, vp, vp, ci]
    n = amp[2] * phase[2] * env[2]
    ref = np.zeros((n, N, N // 2 + 1, 2), dtype=np.float32)
    par = np.zeros((n, 3), dtype=np.float32)
    steps = np.zeros(3, dtype=np.float32)
    got = L.bioem_host_psf_kernels(N, pixelSize, amp[0], amp[1], amp[2], phase[0], phase[1], phase[2], env[0], env[1],
                                   env[2], ref.ctypes.data, par.ctypes.data, steps.ctypes.data, int(device))
    assert got == n
    return ref, par, steps


def volume_element(voluang, gridSpace, maxD, pixelSize, nAmp, gridEnv, gridPhase, sigB, sigDef, sigAmp):
    return load_host_library().bioem_host_volume_element(voluang, gridSpace, maxD, pixelSize, nAmp, gridEnv,
                                                        gridPhase, sigB, sigDef, sigAmp)


def center_model(points):
    pts = np.ascontiguousarray(points.copy())
    nd = load_host_library().bioem_host_center_model(pts.ctypes.data, len(pts))
    return pts, np.float32(nd)


class HostSetup(C.Structure):
    _fields_ = [("pd", ParamDevice), ("nAngles", C.c_int), ("nCTF", C.c_int), ("isQuat", C.c_int),
                ("usepsf", C.c_int), ("shiftX", C.c_int), ("shiftY", C.c_int), ("nocentermass", C.c_int),
                ("pixelSize", C.c_float), ("voluang", C.c_float), ("elecwavel", C.c_float)]


def setup_from_files(paramfile, anglefile=None):
    """readParameters + CalculateGridsParam (+ CalculateRefCTF in CTF mode) of the C++ host layer."""
    L = load_host_library()
    L.bioem_host_setup_from_files.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(HostSetup), C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    S = HostSetup()
    af = anglefile.encode() if anglefile else None
    L.bioem_host_setup_from_files(paramfile.encode(), af, C.byref(S), None, None, None)
    N = S.pd.NumberPixels
    H = N // 2 + 1
    angles = np.zeros((S.nAngles, 4), dtype=np.float32)
    ref = np.zeros((S.nCTF, N, H, 2), dtype=np.float32)
    par = np.zeros((S.nCTF, 3), dtype=np.float32)
    L.bioem_host_setup_from_files(paramfile.encode(), af, C.byref(S), angles.ctypes.data, ref.ctypes.data,
                                  par.ctypes.data)
    return S, angles, ref, par


def read_model(path, isPDB=False, nocentermass=False, cap=1 << 20, isMRC=False, pixelSize=1.0):
    L = load_host_library()
    L.bioem_host_read_model.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_float)]
    L.bioem_host_read_model.restype = C.c_int
    pts = np.zeros(cap, dtype=POINT_DTYPE)
    nd = C.c_float()
    kind = 2 if isMRC else int(bool(isPDB))
    n = L.bioem_host_read_model(path.encode(), kind, int(nocentermass), float(pixelSize), pts.ctypes.data, cap,
                                C.byref(nd))
    return pts[:n].copy(), np.float32(nd.value)


def read_model_volume(path, N, nocentermass=False):
    """the reader of --ModelVolume: an MRC density (mode 2, cubic, side N) as (vol float32 [N, N, N] with its origin at
    voxel (N + 1) // 2 -- the cyclic one-voxel shift of write_mrc_volume undone --, centre float64 [3], its centre of mass in
    voxels relative to the origin (0 with nocentermass), NormDen); any other file ends the process with the reader's fatal"""
    L = load_host_library()
    L.bioem_host_read_model_volume.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.bioem_host_read_model_volume.restype = C.c_int
    vol = np.zeros((N, N, N), dtype=np.float32)
    centre = np.zeros(3, dtype=np.float64)
    nd = C.c_float()
    n = L.bioem_host_read_model_volume(path.encode(), int(N), int(nocentermass), vol.ctypes.data, centre.ctypes.data,
                                       C.byref(nd))
    assert n == N ** 3
    return vol, centre, np.float32(nd.value)


def read_particles(path, N, mode=0, notnormmap=False, cap=4096):
    L = load_host_library()
    L.bioem_host_read_particles.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.bioem_host_read_particles.restype = C.c_int
    maps = np.zeros((cap, N, N), dtype=np.float32)
    n = L.bioem_host_read_particles(path.encode(), mode, N, int(notnormmap), maps.ctypes.data, cap)
    return maps[:n].copy()


class BestParams(C.Structure):
    """the BEST_* file of --PrintBestCalMap as the host layer's parser holds it (phase: the defocus converted)"""
    _fields_ = [("pixelSize", C.c_float), ("N", C.c_int), ("angle", C.c_float * 4), ("doquater", C.c_int),
                ("usepsf", C.c_int), ("withnoise", C.c_int), ("doaaradius", C.c_int), ("printrotmod", C.c_int),
                ("amp", C.c_float), ("phase", C.c_float), ("env", C.c_float), ("ddx", C.c_int), ("ddy", C.c_int),
                ("shiftX", C.c_int), ("shiftY", C.c_int), ("norm", C.c_float), ("offset", C.c_float),
                ("stnoise", C.c_float)]


def read_best_parameters(path):
    """parses a BEST_* file; raises ValueError with the parser's message where the CLI would end with it"""
    L = load_host_library()
    L.bioem_host_read_best_parameters.argtypes = [C.c_char_p, C.POINTER(BestParams), C.c_char_p, C.c_int]
    b = BestParams()
    err = C.create_string_buffer(512)
    if L.bioem_host_read_best_parameters(path.encode(), C.byref(b), err, 512):
        raise ValueError(err.value.decode())
    return b


def write_bestmap(path, image, ddx=0, ddy=0, map_only=False):
    """the BESTMAP text file of the unshifted map image[N, N]"""
    L = load_host_library()
    L.bioem_host_write_bestmap.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    img = np.ascontiguousarray(image, dtype=np.float32)
    assert img.ndim == 2 and img.shape[0] == img.shape[1]
    if L.bioem_host_write_bestmap(path.encode(), img.ctypes.data, img.shape[0], int(ddx), int(ddy), int(bool(map_only))):
        raise RuntimeError("writing %s failed" % path)


def write_mrc_stack(path, maps, batch=64):
    """MRC mode-2 stack of maps[n, N, N] in the storage order the --ReadMRC reader expects"""
    L = load_host_library()
    L.bioem_host_write_mrc_stack.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    m = np.ascontiguousarray(maps, dtype=np.float32)
    assert m.ndim == 3 and m.shape[1] == m.shape[2]
    if L.bioem_host_write_mrc_stack(path.encode(), m.ctypes.data, m.shape[0], m.shape[1], int(batch)):
        raise RuntimeError("writing %s failed" % path)


def write_ctf_prob(path, table, ctfParam, angles, Ntotpi, volu, usepsf=False, elecwavel=0.019688, isQuat=True,
                   angles_per_map=0, volu_per_map=None):
    """the --ProbCTF text file of a CTF table [nCTF, nMaps] (Engine.ctf_table, merge_ctf_tables): the writer the CLI
    uses.  angles [n, 4]: the list `orient` indexes, one for all maps, or angles_per_map entries per map.  Raises
    ValueError with the writer's message where the CLI would end with it (an entry no comparison touched)."""
    from .engine import PROB_MAP_DTYPE
    L = load_host_library()
    L.bioem_host_write_ctf_prob.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                            C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_char_p,
                                            C.c_int]
    tab = np.ascontiguousarray(table, dtype=PROB_MAP_DTYPE)
    assert tab.ndim == 2
    par = np.ascontiguousarray(ctfParam, dtype=np.float32)
    assert par.shape == (tab.shape[0], 3)
    ang = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
    vpm = None if volu_per_map is None else np.ascontiguousarray(volu_per_map, dtype=np.float32)
    assert vpm is None or vpm.shape == (tab.shape[1],)
    err = C.create_string_buffer(512)
    if L.bioem_host_write_ctf_prob(path.encode(), tab.ctypes.data, tab.shape[0], tab.shape[1], par.ctypes.data,
                                   int(bool(usepsf)), float(elecwavel), int(bool(isQuat)), ang.ctypes.data,
                                   int(angles_per_map), float(Ntotpi), float(volu),
                                   None if vpm is None else vpm.ctypes.data, err, 512):
        raise ValueError(err.value.decode())


def write_best_frc(path, sums, N, pixelSize):
    """the --BestFRC text file of ring sums [nMaps, ring_count(N)] (Engine.best_match_rings): the writer the CLI uses;
    bioem_amd.best_frc.parse reads it back"""
    from .engine import RING_SUMS_DTYPE
    L = load_host_library()
    L.bioem_host_write_best_frc.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_char_p, C.c_int]
    t = np.ascontiguousarray(sums, dtype=RING_SUMS_DTYPE)
    assert t.ndim == 2
    err = C.create_string_buffer(512)
    if L.bioem_host_write_best_frc(path.encode(), t.ctypes.data, t.shape[0], int(N), float(pixelSize), err, 512):
        raise ValueError(err.value.decode())


def view_groups(pmap, nOrient, min_count=2):
    """the grouping the CLI uses for --ViewAverages (view_groups_by_orientation): (group_of int32 [nMaps], group_orient
    int32 [nViews]) from the arg-max orientation of the records; bioem_amd.view_average.groups_by_orientation restates it"""
    from .engine import PROB_MAP_DTYPE
    L = load_host_library()
    L.bioem_host_view_groups.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    pmap = np.ascontiguousarray(pmap, dtype=PROB_MAP_DTYPE)
    group_of = np.zeros(len(pmap), dtype=np.int32)
    group_orient = np.zeros(max(int(nOrient), 1), dtype=np.int32)
    n = L.bioem_host_view_groups(pmap.ctypes.data, len(pmap), int(nOrient), int(min_count), group_of.ctypes.data,
                                 group_orient.ctypes.data, len(group_orient))
    return group_of, group_orient[:n].copy()


def write_view_averages(path, rings, group_orient, counts, angles, doquater, N, pixelSize, min_count=2, wiener=0.1):
    """the --ViewAverages text file of ring sums [nViews, ring_count(N)] (Engine.view_averages): the writer the CLI uses;
    bioem_amd.view_average.parse reads it back.  angles: the orientation list [nOrient, 4] group_orient indexes."""
    from .engine import RING_SUMS_DTYPE
    L = load_host_library()
    L.bioem_host_write_view_averages.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_float, C.c_int, C.c_double, C.c_char_p, C.c_int]
    t = np.ascontiguousarray(rings, dtype=RING_SUMS_DTYPE)
    go = np.ascontiguousarray(group_orient, dtype=np.int32)
    cn = np.ascontiguousarray(counts, dtype=np.int32)
    ang = np.ascontiguousarray(angles, dtype=np.float32)
    assert t.ndim == 2 and go.shape == cn.shape == (t.shape[0],) and ang.ndim == 2 and ang.shape[1] == 4
    err = C.create_string_buffer(512)
    if L.bioem_host_write_view_averages(path.encode(), t.ctypes.data, t.shape[0], go.ctypes.data, cn.ctypes.data, ang.ctypes.data,
                                        int(bool(doquater)), int(N), float(pixelSize), int(min_count), float(wiener), err, 512):
        raise ValueError(err.value.decode())


def write_reconstruction(path, specA, specB, N, pixelSize, wiener=0.1, views=0, particles=0, tau=0.0):
    """the --Reconstruct text file from the two half-set spectra complex128 [N, N, H] (Engine.reconstruct): the shell sums and
    the writer the CLI uses; bioem_amd.reconstruct.parse reads it back"""
    L = load_host_library()
    L.bioem_host_write_reconstruction.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_double,
                                                  C.c_longlong, C.c_longlong, C.c_double, C.c_char_p, C.c_int]
    A = np.ascontiguousarray(specA, dtype=np.complex128)
    B = np.ascontiguousarray(specB, dtype=np.complex128)
    assert A.shape == B.shape == (N, N, N // 2 + 1)
    err = C.create_string_buffer(512)
    if L.bioem_host_write_reconstruction(path.encode(), A.ctypes.data, B.ctypes.data, int(N), float(pixelSize), float(wiener),
                                         int(views), int(particles), float(tau), err, 512):
        raise ValueError(err.value.decode())


def write_mrc_volume(path, vol, pixelSize):
    """a volume float32 [N, N, N] as the MRC file of --Reconstruct (the writer the CLI uses): read_model(isMRC=True) places
    every point where the reconstruction has it; bioem_amd.reconstruct.read_mrc reads the volume back"""
    L = load_host_library()
    L.bioem_host_write_mrc_volume.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_float, C.c_char_p, C.c_int]
    v = np.ascontiguousarray(vol, dtype=np.float32)
    assert v.ndim == 3 and v.shape == (v.shape[0],) * 3
    err = C.create_string_buffer(512)
    if L.bioem_host_write_mrc_volume(path.encode(), v.ctypes.data, v.shape[0], float(pixelSize), err, 512):
        raise ValueError(err.value.decode())


def write_best_window(path, logp, shifts, orient, conv, ctfParam, numconst, usepsf=False, elecwavel=0.019866):
    """the --BestWindow text file of window tables [nMaps, nd, nd] (Engine.best_match_window) at the shifts [nd]: the
    writer the CLI uses; bioem_amd.best_window.parse reads it back.  orient, conv [nMaps]: the records' pair (orient < 0:
    a particle without a table); ctfParam [nCTF, 3]; numconst: the constant of every particle's LogProb (a scalar or
    [nMaps])"""
    L = load_host_library()
    vp = C.c_void_p
    L.bioem_host_write_best_window.argtypes = [C.c_char_p, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_float, vp,
                                               C.c_char_p, C.c_int]
    t = np.ascontiguousarray(logp, dtype=np.float64)
    X = np.ascontiguousarray(shifts, dtype=np.int32)
    assert t.ndim == 3 and t.shape[1:] == (len(X), len(X))
    o = np.ascontiguousarray(orient, dtype=np.int32)
    c = np.ascontiguousarray(conv, dtype=np.int32)
    k = np.ascontiguousarray(ctfParam, dtype=np.float32)
    nc = np.ascontiguousarray(np.broadcast_to(np.asarray(numconst, dtype=np.float64), (t.shape[0],)))
    assert o.shape == (t.shape[0],) and c.shape == o.shape and k.ndim == 2 and k.shape[1] == 3
    err = C.create_string_buffer(512)
    if L.bioem_host_write_best_window(path.encode(), t.ctypes.data, X.ctypes.data, len(X), t.shape[0], o.ctypes.data,
                                      c.ctypes.data, k.ctypes.data, int(bool(usepsf)), float(elecwavel), nc.ctypes.data,
                                      err, 512):
        raise ValueError(err.value.decode())


def write_orient_stats(path, sums, angles, doquater, numconst):
    """the --OrientStats text file of orientation sums [nMaps] (Engine.orientation_sums) against the orientation list
    `angles` [nO, 4]: the writer the CLI uses; bioem_amd.orient_stats.parse reads it back"""
    from .engine import ORIENT_SUMS_DTYPE
    L = load_host_library()
    L.bioem_host_write_orient_stats.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double,
                                                C.c_char_p, C.c_int]
    t = np.ascontiguousarray(sums, dtype=ORIENT_SUMS_DTYPE)
    a = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
    assert t.ndim == 1
    err = C.create_string_buffer(512)
    if L.bioem_host_write_orient_stats(path.encode(), t.ctypes.data, t.shape[0], a.ctypes.data, int(bool(doquater)),
                                       float(numconst), err, 512):
        raise ValueError(err.value.decode())


def jacobi4(A):
    """eigenvalues (descending) and eigenvectors (row k belongs to eigenvalue k) of a symmetric 4 x 4 matrix by the Jacobi
    solver of the --OrientStats writer"""
    L = load_host_library()
    L.bioem_host_jacobi4.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.bioem_host_jacobi4.restype = None
    a = np.ascontiguousarray(A, dtype=np.float64)
    assert a.shape == (4, 4)
    w, v = np.zeros(4), np.zeros((4, 4))
    L.bioem_host_jacobi4(a.ctypes.data, w.ctypes.data, v.ctypes.data)
    return w, v


def write_orient_occupancy(path, occ, angles, doquater, nCounted, fits=None):
    """the --OrientOccupancy text file of an occupancy [nO] (Engine.orientation_occupancy) against the orientation list
    `angles` [nO, 4]; fits: None or [T, 2] of (logLikelihood, nEffViews), the FIT lines: the writer the CLI uses;
    bioem_amd.orient_occupancy.parse reads it back"""
    from .engine import ORIENT_OCC_DTYPE
    L = load_host_library()
    L.bioem_host_write_orient_occupancy.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                                    C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    t = np.ascontiguousarray(occ, dtype=ORIENT_OCC_DTYPE)
    a = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
    assert t.ndim == 1 and len(a) >= len(t)
    F = np.ascontiguousarray(fits if fits is not None else np.zeros((0, 2)), dtype=np.float64).reshape(-1, 2)
    err = C.create_string_buffer(512)
    if L.bioem_host_write_orient_occupancy(path.encode(), t.ctypes.data, t.shape[0], a.ctypes.data, int(bool(doquater)),
                                           int(nCounted), F.ctypes.data if len(F) else None, len(F), err, 512):
        raise ValueError(err.value.decode())


def write_orient_prior(path, angles, doquater, logPrior):
    """the FILE_prior of --FitOrientPrior: the orientation list in the --ReadOrientation format with the additive log
    prior as its last column (clamped to [orient_occupancy.L0, 0], %12.5e)"""
    L = load_host_library()
    L.bioem_host_write_orient_prior.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    a = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
    lp = np.ascontiguousarray(logPrior, dtype=np.float64)
    assert lp.shape == (len(a),)
    err = C.create_string_buffer(512)
    if L.bioem_host_write_orient_prior(path.encode(), a.ctypes.data, len(a), int(bool(doquater)), lp.ctypes.data, err, 512):
        raise ValueError(err.value.decode())


def occ_next_prior(occ, nCounted):
    """the EM update of --FitOrientPrior as the CLI forms it: (log prior [nO], the floor written where occ = 0)"""
    from .engine import ORIENT_OCC_DTYPE
    L = load_host_library()
    L.bioem_host_occ_next_prior.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    L.bioem_host_occ_next_prior.restype = C.c_double
    t = np.ascontiguousarray(occ, dtype=ORIENT_OCC_DTYPE)
    lp = np.zeros(len(t))
    floor = L.bioem_host_occ_next_prior(t.ctypes.data, len(t), int(nCounted), lp.ctypes.data)
    return lp, floor


def read_orientation_list(paramfile, anglefile, cap=1 << 20):
    """the orientation list as the host parameter reader keeps it (readParameters + CalculateGridsParam): angles
    float32 [n, 4] and, under PRIOR_ANGLES, the prior column float32 [n], else None"""
    L = load_host_library()
    L.bioem_host_read_orientation_list.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.POINTER(C.c_int)]
    L.bioem_host_read_orientation_list.restype = C.c_int
    has = C.c_int(0)
    af = anglefile.encode() if anglefile else None
    n = L.bioem_host_read_orientation_list(paramfile.encode(), af, None, None, 0, C.byref(has))
    assert n <= cap
    ang = np.zeros((n, 4), dtype=np.float32)
    pri = np.zeros(n, dtype=np.float32)
    L.bioem_host_read_orientation_list(paramfile.encode(), af, ang.ctypes.data, pri.ctypes.data, n, C.byref(has))
    return ang, (pri if has.value else None)


def ctf_kernel_list(N, pixelSize, triples, usepsf=False, device=0):
    """the kernels float32 [G, N, H, 2] of G triples (amp, phase, env) in the reference's internal units: per triple the
    expression of ctf_kernels, so a triple of the grid carries the grid kernel's bits.  PSF mode transforms on `device`."""
    L = load_host_library()
    L.bioem_host_ctf_kernel_list.argtypes = [C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    t = np.ascontiguousarray(triples, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((len(t), int(N), int(N) // 2 + 1, 2), dtype=np.float32)
    if L.bioem_host_ctf_kernel_list(int(N), float(pixelSize), int(bool(usepsf)), t.ctypes.data, len(t), out.ctypes.data,
                                    int(device)):
        raise ValueError("ctf_kernel_list: N < 2 or no triples")
    return out


def ctf_scan_refine(start, step, n, k):
    """the --CTFScan candidates as the CLI forms them (ctf_scan_refine): (triples float32 [G, 3], counts int32 [3]) from the
    grid's start, step and point count per axis (amp, phase, env); ValueError for a factor the CLI refuses"""
    L = load_host_library()
    L.bioem_host_ctf_scan_refine.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(start, dtype=np.float32)
    g = np.ascontiguousarray(step, dtype=np.float32)
    m = np.ascontiguousarray(n, dtype=np.int32)
    assert a.shape == g.shape == m.shape == (3,)
    counts = np.zeros(3, dtype=np.int32)
    G = L.bioem_host_ctf_scan_refine(a.ctypes.data, g.ctypes.data, m.ctypes.data, int(k), counts.ctypes.data, None)
    if G < 0:
        raise ValueError("factor %r is not one of 1, 2, 4, 8, 16" % (k,))
    t = np.zeros((G, 3), dtype=np.float32)
    assert L.bioem_host_ctf_scan_refine(a.ctypes.data, g.ctypes.data, m.ctypes.data, int(k), counts.ctypes.data,
                                        t.ctypes.data) == G
    return t, counts


def write_ctf_scan(path, logp, triples, counts, orient, shiftX, shiftY, numconst, usepsf=False, elecwavel=0.019866):
    """the --CTFScan text file of scan tables [nMaps, G] (Engine.best_match_ctf_scan) over the candidates triples [G, 3]
    with counts [3] values per axis: the writer the CLI uses; bioem_amd.ctf_scan.parse reads it back.  orient, shiftX,
    shiftY [nMaps]: the records (orient < 0: a particle without a table); numconst: the constant of every particle's
    LogProb (a scalar or [nMaps])"""
    L = load_host_library()
    vp = C.c_void_p
    L.bioem_host_write_ctf_scan.argtypes = [C.c_char_p, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, vp, C.c_char_p,
                                            C.c_int]
    t = np.ascontiguousarray(logp, dtype=np.float64)
    k = np.ascontiguousarray(triples, dtype=np.float32)
    cn = np.ascontiguousarray(counts, dtype=np.int32)
    assert t.ndim == 2 and k.shape == (t.shape[1], 3) and cn.shape == (3,) and int(cn.prod()) == t.shape[1]
    o = np.ascontiguousarray(orient, dtype=np.int32)
    sx = np.ascontiguousarray(shiftX, dtype=np.int32)
    sy = np.ascontiguousarray(shiftY, dtype=np.int32)
    nc = np.ascontiguousarray(np.broadcast_to(np.asarray(numconst, dtype=np.float64), (t.shape[0],)))
    assert o.shape == sx.shape == sy.shape == (t.shape[0],)
    err = C.create_string_buffer(512)
    if L.bioem_host_write_ctf_scan(path.encode(), t.ctypes.data, k.ctypes.data, cn.ctypes.data, t.shape[0], o.ctypes.data,
                                   sx.ctypes.data, sy.ctypes.data, int(bool(usepsf)), float(elecwavel), nc.ctypes.data, err,
                                   512):
        raise ValueError(err.value.decode())


def write_model_gradient(path, points, acc, nonfinite=0):
    """the --ModelGradient text file of the sums acc (GRAD_POINT_DTYPE [nPts], Engine.model_gradient's "points") over the
    model's points (POINT_DTYPE [nPts]): the writer the CLI uses; bioem_amd.model_gradient.parse reads it back"""
    L = load_host_library()
    vp = C.c_void_p
    L.bioem_host_write_model_gradient.argtypes = [C.c_char_p, vp, vp, C.c_int, C.c_int, C.c_char_p, C.c_int]
    p = np.ascontiguousarray(points)
    a = np.ascontiguousarray(acc)
    assert p.dtype.itemsize == 24 and a.dtype.itemsize == 32 and p.shape == a.shape and p.ndim == 1
    err = C.create_string_buffer(512)
    if L.bioem_host_write_model_gradient(path.encode(), p.ctypes.data, a.ctypes.data, len(p), int(nonfinite), err, 512):
        raise ValueError(err.value.decode())
