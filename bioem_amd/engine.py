"""ctypes binding of include/bioem_hip.h (libbioem_hip.so).  No fallback path: if the HIP library
cannot be loaded this module raises."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

PROB_MAP_DTYPE = np.dtype([("Total", "<f8"), ("Constoadd", "<f8"), ("cent_x", "<i4"), ("cent_y", "<i4"),
                           ("orient", "<i4"), ("conv", "<i4"), ("norm", "<f4"), ("mu", "<f4")])
PROB_ANGLE_DTYPE = np.dtype([("forAngles", "<f8"), ("ConstAngle", "<f8")])
PARAM5_DTYPE = np.dtype([("amp", "<f4"), ("pha", "<f4"), ("env", "<f4"), ("sumC", "<f4"), ("sumsquareC", "<f4")])
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("quat4", "<f4"), ("radius", "<f4"), ("density", "<f4")])
PHASE_RECORD_DTYPE = np.dtype([("phase", "<i4"), ("iOrientBegin", "<i4"), ("iOrientEnd", "<i4"), ("iConvBegin", "<i4"),
                               ("iConvEnd", "<i4"), ("pad", "<i4"), ("seconds", "<f8")])
CANDIDATE_DTYPE = np.dtype([("forAngles", "<f8"), ("ConstAngle", "<f8"), ("logp", "<f8"), ("orient", "<i4"),
                            ("pad", "<i4")])
RING_SUMS_DTYPE = np.dtype([("cross", "<f8"), ("powParticle", "<f8"), ("powModel", "<f8")])
ORIENT_SUMS_DTYPE = np.dtype([("m", "<f8"), ("omax", "<f8"), ("count", "<f8"), ("hasMoments", "<f8"), ("S0", "<f8"),
                              ("S1", "<f8"), ("S2", "<f8"), ("Q", "<f8", (10,))])
ORIENT_OCC_DTYPE = np.dtype([("occ", "<f8"), ("occ2", "<f8"), ("wmax", "<f8"), ("pmax", "<f8"), ("count", "<f8"),
                             ("hard", "<f8")])
WINDOW_REQUEST_DTYPE = np.dtype([("particle", "<i4"), ("orient", "<i4"), ("conv", "<i4")])
SCAN_REQUEST_DTYPE = np.dtype([("particle", "<i4"), ("orient", "<i4"), ("shiftX", "<i4"), ("shiftY", "<i4")])
GRAD_REQUEST_DTYPE = np.dtype([("particle", "<i4"), ("orient", "<i4"), ("conv", "<i4"), ("shiftX", "<i4"), ("shiftY", "<i4")])
# a row of bioem_hip_pose_gradient: d log P / d R[i][j] (rows 0 and 1), d log P / d (shiftX, shiftY), <C, A_r>, the matrix
POSE_GRAD_DTYPE = np.dtype([("J", "<f8", (2, 3)), ("T", "<f8", (2,)), ("dot", "<f8"), ("R", "<f8", (3, 3))])
# a row of bioem_hip_ctf_gradient: theta = (amp, pha, env) of the request's CTF set, the twenty sums (ss0, cc0, U[3], V[3],
# UU[6], VV[6]), gradient and Hessian of log P with respect to theta, the data's part and that of -prior apart; the Hessian's
# upper triangle in the order aa, ap, ae, pp, pe, ee, the prior's diagonal
CTF_GRAD_DTYPE = np.dtype([("theta", "<f8", (3,)), ("sums", "<f8", (20,)), ("gData", "<f8", (3,)), ("gPrior", "<f8", (3,)),
                           ("HData", "<f8", (6,)), ("HPrior", "<f8", (3,))])
SOFT_MEMBER_DTYPE = np.dtype([("particle", "<i4"), ("group", "<i4"), ("conv", "<i4"), ("pad", "<i4"), ("s2", "<f8"),
                              ("b", "<f8"), ("mass", "<f8")])
GRAD_POINT_DTYPE = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("sumw", "<f8"), ("count", "<i8")])
MIN_PROB = -999999.0
RECON_CORRECT, RECON_NO_CULL = 1, 2   # BIOEM_HIP_RECON_* of include/bioem_hip.h
VOLUME_PRECORRECT = 1                 # BIOEM_HIP_VOLUME_PRECORRECT


class ParamDevice(C.Structure):
    """bioem_hip_param_device == bioem_param_device (reference include/param.h:26-47)."""
    _fields_ = [("maxDisplaceCenter", C.c_int), ("GridSpaceCenter", C.c_int), ("NumberPixels", C.c_int),
                ("NumberFFTPixels1D", C.c_int), ("NxDisp", C.c_int), ("NtotDisp", C.c_int),
                ("Ntotpi", C.c_float), ("volu", C.c_float), ("sigmaPriorbctf", C.c_float),
                ("sigmaPriordefo", C.c_float), ("Priordefcent", C.c_float), ("sigmaPrioramp", C.c_float),
                ("Priorampcent", C.c_float), ("writeAngles", C.c_int), ("tousepsf", C.c_int)]


def lib_path():
    # BIOEM_HIP_LIBRARY: an experiment build of the same library (scripts/slim_build.sh) for same-box A/B runs
    alt = os.environ.get("BIOEM_HIP_LIBRARY")
    if alt:
        return alt if os.path.isabs(alt) else os.path.join(os.path.dirname(HERE), alt)
    return os.path.join(HERE, "lib", "libbioem_hip.so")


_lib = None


def load_library():
    """Loads libbioem_hip.so and declares every entry point of include/bioem_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError("HIP engine not built: %s is missing (run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` or `make -C bioem_amd/csrc`); there is no CPU fallback" % path)
    L = C.CDLL(path)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.bioem_hip_device_count.restype = ci
    L.bioem_hip_create.argtypes = [C.POINTER(vp), ci, C.POINTER(ParamDevice), ci, ci, ci, ci]
    L.bioem_hip_create_shard.argtypes = [C.POINTER(vp), ci, C.POINTER(ParamDevice), ci, ci, ci, ci, ci, ci]
    L.bioem_hip_destroy.argtypes = [vp]
    L.bioem_hip_last_error.argtypes = [vp]
    L.bioem_hip_last_error.restype = C.c_char_p
    L.bioem_hip_upload_particles.argtypes = [vp, vp, vp, vp]
    L.bioem_hip_upload_particle_maps.argtypes = [vp, vp]
    L.bioem_hip_upload_ctf.argtypes = [vp, vp, vp]
    L.bioem_hip_upload_model.argtypes = [vp, vp, ci, cf, cf, ci, ci]
    L.bioem_hip_upload_orientations.argtypes = [vp, vp, ci, ci]
    # (a build from before these two entries, loaded through BIOEM_HIP_LIBRARY as the other side of an A/B run, still
    # serves every other entry; the Engine methods that need them raise AttributeError on it)
    if hasattr(L, "bioem_hip_upload_particle_orientations"):
        L.bioem_hip_upload_particle_orientations.argtypes = [vp, vp, ci, ci]
        L.bioem_hip_compare_own_orientations.argtypes = [vp, ci, ci]
    if hasattr(L, "bioem_hip_upload_particle_orientation_lists"):
        L.bioem_hip_upload_particle_orientation_lists.argtypes = [vp, vp, vp, ci]
        L.bioem_hip_plan_own.argtypes = [ci, ci, ci, ci, C.c_char_p, ci]
        L.bioem_hip_own_kernel_signature.argtypes = [vp]
        L.bioem_hip_own_kernel_signature.restype = C.c_char_p
        L.bioem_hip_set_own_launch.argtypes = [vp, ci]
    if hasattr(L, "bioem_hip_set_compare_variant"):
        L.bioem_hip_set_compare_variant.argtypes = [vp, ci]
    if hasattr(L, "bioem_hip_render_best_maps"):
        L.bioem_hip_render_best_maps.argtypes = [vp, vp, ci, ci, ci, vp]
    if hasattr(L, "bioem_hip_enable_ctf_table"):
        L.bioem_hip_enable_ctf_table.argtypes = [vp, ci]
        L.bioem_hip_ctf_table.argtypes = [vp, vp]
    if hasattr(L, "bioem_hip_best_match_rings"):
        L.bioem_hip_ring_count.argtypes = [ci]
        L.bioem_hip_best_match_rings.argtypes = [vp, vp, ci, ci, ci, vp]
        L.bioem_hip_debug_ring_sums.argtypes = [vp, vp, vp, vp, ci, vp]
    if hasattr(L, "bioem_hip_window_posterior"):
        L.bioem_hip_window_count.argtypes = [ci, ci, ci, ci]
        L.bioem_hip_window_offsets.argtypes = [ci, ci, ci, ci, vp, ci]
        L.bioem_hip_window_posterior.argtypes = [vp, vp, ci, ci, vp, vp, vp]
        L.bioem_hip_debug_window.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp]
    if hasattr(L, "bioem_hip_ctf_scan"):
        L.bioem_hip_ctf_scan.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp, vp, vp]
        L.bioem_hip_debug_ctf_scan.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp]
    if hasattr(L, "bioem_hip_model_gradient"):
        L.bioem_hip_model_gradient.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, vp]
        L.bioem_hip_debug_grad_image.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
        L.bioem_hip_debug_grad_gather.argtypes = [vp, vp, ci, ci, vp]
    if hasattr(L, "bioem_hip_orientation_sums"):
        L.bioem_hip_orientation_sums.argtypes = [vp, vp, ci, ci, ci, vp]
        L.bioem_hip_merge_orient_sums_host.argtypes = [ci, ci, C.POINTER(vp), vp]
        L.bioem_hip_debug_orient_sums.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp]
        L.bioem_hip_debug_orient_sums_own.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp]
    if hasattr(L, "bioem_hip_orientation_occupancy"):
        L.bioem_hip_orientation_occupancy.argtypes = [vp, vp, vp, ci, ci, vp]
        L.bioem_hip_debug_orient_occupancy.argtypes = [vp, vp, ci, ci, vp, vp, ci, ci, ci, vp]
    if hasattr(L, "bioem_hip_view_sums"):
        L.bioem_hip_view_sums.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp]
        L.bioem_hip_view_averages.argtypes = [vp, vp, vp, vp, vp, ci, C.c_double, ci, ci, vp, vp, vp]
        L.bioem_hip_debug_view_sums.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
    if hasattr(L, "bioem_hip_reconstruct"):
        L.bioem_hip_reconstruct.argtypes = [vp, vp, vp, vp, vp, ci, C.c_double, ci, vp, vp, vp, vp]
        L.bioem_hip_debug_reconstruct.argtypes = [vp, vp, vp, vp, ci, ci, C.c_double, ci, vp, vp, vp, vp]
    if hasattr(L, "bioem_hip_view_sums_soft"):
        L.bioem_hip_view_sums_soft.argtypes = [vp, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp]
        L.bioem_hip_debug_view_sums_soft.argtypes = [vp, vp, ci, vp, vp, ci, vp, ci, ci, vp, vp, vp]
        L.bioem_hip_reconstruct_soft.argtypes = [vp, vp, vp, ci, vp, ci, vp, ci, C.c_double, ci, vp, vp, vp, vp]
    if hasattr(L, "bioem_hip_upload_model_volume"):
        L.bioem_hip_upload_model_spectrum.argtypes = [vp, vp, ci, vp, ci, ci]
        L.bioem_hip_upload_model_volume.argtypes = [vp, vp, ci, ci, vp, ci, ci]
        L.bioem_hip_debug_slices.argtypes = [vp, vp, ci, ci, vp]
    if hasattr(L, "bioem_hip_volume_gradient"):
        L.bioem_hip_volume_gradient.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.bioem_hip_debug_volume_backproject.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp]
        L.bioem_hip_debug_volume_adjoint.argtypes = [vp, vp, vp]
    if hasattr(L, "bioem_hip_pose_gradient"):
        L.bioem_hip_pose_gradient.argtypes = [vp, vp, ci, ci, vp, vp, vp]
        L.bioem_hip_debug_pose_sums.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    if hasattr(L, "bioem_hip_ctf_gradient"):
        L.bioem_hip_ctf_gradient.argtypes = [vp, vp, ci, ci, cf, vp, vp, vp]
        L.bioem_hip_debug_ctf_gradient.argtypes = [vp, vp, vp, vp, vp, ci, cf, vp, vp]
    L.bioem_hip_host_alloc.argtypes = [C.c_size_t]
    L.bioem_hip_host_alloc.restype = vp
    L.bioem_hip_host_free.argtypes = [vp]
    L.bioem_hip_prob_size.argtypes = [ci, ci, ci]
    L.bioem_hip_prob_size.restype = C.c_size_t
    L.bioem_hip_start_run.argtypes = [vp, vp]
    L.bioem_hip_compare.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp]
    L.bioem_hip_project_convolve_compare.argtypes = [vp, ci, ci]
    L.bioem_hip_project_convolve_compare_ctf.argtypes = [vp, ci, ci, ci, ci]
    L.bioem_hip_project.argtypes = [vp, ci, ci, ci]
    L.bioem_hip_convolve.argtypes = [vp, ci, ci, ci]
    L.bioem_hip_compare_device.argtypes = [vp, ci]
    L.bioem_hip_max_batch.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.bioem_hip_finish_run.argtypes = [vp, vp]
    L.bioem_hip_set_phase_timing.argtypes = [vp, ci]
    L.bioem_hip_phase_records.argtypes = [vp, vp, ci, C.POINTER(ci)]
    L.bioem_hip_topk_angles.argtypes = [vp, ci, C.c_double, vp]
    L.bioem_hip_merge_topk_host.argtypes = [ci, ci, ci, C.POINTER(vp), vp]
    L.bioem_hip_merge_candidates.argtypes = [vp, ci, C.c_double, vp]
    L.bioem_hip_merge_topk_host_wide.argtypes = [ci, ci, ci, ci, C.POINTER(vp), vp]
    L.bioem_hip_debug_topk.argtypes = [vp, vp, ci, ci, ci, ci, ci, C.c_double, vp]
    L.bioem_hip_debug_merge_gathered.argtypes = [vp, vp, ci, ci, vp, vp]
    L.bioem_hip_merge.argtypes = [C.POINTER(vp), ci, vp, ci, C.c_double, vp]
    L.bioem_hip_merge_host.argtypes = [ci, ci, ci, ci, C.POINTER(vp), vp]
    L.bioem_hip_debug_projection.argtypes = [vp, ci, vp]
    if hasattr(L, "bioem_hip_debug_projection_maps"):
        L.bioem_hip_debug_projection_maps.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp]
        L.bioem_hip_debug_stamps.argtypes = [vp, vp, C.POINTER(ci)]
    L.bioem_hip_debug_convolution.argtypes = [vp, ci, ci, vp, C.POINTER(cf), C.POINTER(cf)]
    if hasattr(L, "bioem_hip_debug_convolve_batch"):
        L.bioem_hip_debug_convolve_batch.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp]
    L.bioem_hip_debug_particles.argtypes = [vp, vp, vp, vp]
    L.bioem_hip_debug_direct_conv.argtypes = [vp, vp, ci, vp, vp]
    L.bioem_hip_kernel_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.bioem_hip_reset_kernel_stats.argtypes = [vp]
    L.bioem_hip_uses_fast_path.argtypes = [vp]
    L.bioem_hip_kernel_name.argtypes = [vp]
    L.bioem_hip_kernel_name.restype = C.c_char_p
    L.bioem_hip_kernel_signature.argtypes = [vp]
    L.bioem_hip_kernel_signature.restype = C.c_char_p
    L.bioem_hip_plan.argtypes = [ci, ci, ci, ci, C.c_char_p, ci]
    L.bioem_hip_synchronize.argtypes = [vp]
    L.bioem_hip_r2c.argtypes = [ci, ci, ci, vp, vp]
    _lib = L
    return L


EXPORTS = ["bioem_hip_device_count", "bioem_hip_create", "bioem_hip_create_shard", "bioem_hip_destroy",
           "bioem_hip_last_error", "bioem_hip_project_convolve_compare_ctf", "bioem_hip_topk_angles",
           "bioem_hip_merge_topk_host", "bioem_hip_merge", "bioem_hip_merge_candidates", "bioem_hip_merge_topk_host_wide",
           "bioem_hip_debug_topk", "bioem_hip_debug_merge_gathered",
           "bioem_hip_upload_particles", "bioem_hip_upload_particle_maps", "bioem_hip_upload_ctf",
           "bioem_hip_upload_model", "bioem_hip_upload_orientations", "bioem_hip_host_alloc",
           "bioem_hip_host_free", "bioem_hip_prob_size", "bioem_hip_start_run", "bioem_hip_compare",
           "bioem_hip_project_convolve_compare", "bioem_hip_finish_run", "bioem_hip_merge_host",
           "bioem_hip_debug_projection", "bioem_hip_debug_convolution", "bioem_hip_debug_particles",
           "bioem_hip_kernel_stats", "bioem_hip_reset_kernel_stats", "bioem_hip_uses_fast_path",
           "bioem_hip_kernel_name", "bioem_hip_kernel_signature", "bioem_hip_plan",
           "bioem_hip_synchronize", "bioem_hip_r2c", "bioem_hip_project", "bioem_hip_convolve",
           "bioem_hip_compare_device", "bioem_hip_max_batch", "bioem_hip_set_phase_timing", "bioem_hip_phase_records",
           "bioem_hip_upload_particle_orientations", "bioem_hip_compare_own_orientations",
           "bioem_hip_upload_particle_orientation_lists", "bioem_hip_plan_own", "bioem_hip_own_kernel_signature",
           "bioem_hip_set_own_launch", "bioem_hip_render_best_maps", "bioem_hip_enable_ctf_table",
           "bioem_hip_ctf_table", "bioem_hip_ring_count", "bioem_hip_best_match_rings", "bioem_hip_debug_ring_sums",
           "bioem_hip_window_count", "bioem_hip_window_offsets", "bioem_hip_window_posterior", "bioem_hip_debug_window",
           "bioem_hip_ctf_scan", "bioem_hip_debug_ctf_scan",
           "bioem_hip_model_gradient", "bioem_hip_debug_grad_image", "bioem_hip_debug_grad_gather",
           "bioem_hip_orientation_sums", "bioem_hip_merge_orient_sums_host", "bioem_hip_debug_orient_sums",
           "bioem_hip_debug_orient_sums_own", "bioem_hip_orientation_occupancy", "bioem_hip_debug_orient_occupancy",
           "bioem_hip_view_sums", "bioem_hip_view_averages", "bioem_hip_debug_view_sums",
           "bioem_hip_reconstruct", "bioem_hip_debug_reconstruct",
           "bioem_hip_view_sums_soft", "bioem_hip_debug_view_sums_soft", "bioem_hip_reconstruct_soft",
           "bioem_hip_set_compare_variant", "bioem_hip_debug_projection_maps", "bioem_hip_debug_stamps",
           "bioem_hip_debug_convolve_batch", "bioem_hip_debug_direct_conv",
           "bioem_hip_upload_model_spectrum", "bioem_hip_upload_model_volume", "bioem_hip_debug_slices",
           "bioem_hip_volume_gradient", "bioem_hip_debug_volume_backproject", "bioem_hip_debug_volume_adjoint",
           "bioem_hip_pose_gradient", "bioem_hip_debug_pose_sums",
           "bioem_hip_ctf_gradient", "bioem_hip_debug_ctf_gradient"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _spectra(a):
    """spectra float32 [..., 2], or complex [...] viewed as such"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = np.ascontiguousarray(a.astype(np.complex64)).view(np.float32).reshape(a.shape + (2,))
    return np.ascontiguousarray(a, dtype=np.float32)


def _pmap(pmap, n):
    """the map entries of a probability block: PROB_MAP_DTYPE [n], contiguous"""
    pmap = np.ascontiguousarray(pmap, dtype=PROB_MAP_DTYPE)
    assert pmap.shape == (n,)
    return pmap


def _vector(v, n):
    """an optional prior or weight vector: None, or float64 [n], contiguous"""
    if v is None:
        return None
    v = np.ascontiguousarray(v, dtype=np.float64)
    assert v.shape == (n,), v.shape
    return v


def _requests(requests, dtype):
    """requests of a request dtype as a contiguous [n] array of it: such an array itself, or an [n, k] integer array (a
    list of tuples) with the columns in the order of dtype.names"""
    r = np.asarray(requests)
    if r.dtype != dtype:
        r = np.asarray(r, dtype=np.int32)
        if r.ndim == 2 and r.shape[1] != len(dtype.names):
            raise ValueError("%d columns for the requests (%s)" % (r.shape[1], ", ".join(dtype.names)))
        r = r.reshape(-1, len(dtype.names))
        q = np.zeros(len(r), dtype=dtype)
        for i, f in enumerate(dtype.names):
            q[f] = r[:, i]
        r = q
    return np.ascontiguousarray(r.reshape(-1))


def _match_requests(pmap, p0, p1, dtype):
    """the requests of a request dtype for the best records of particles [p0, p1) of pmap (PROB_MAP_DTYPE): every field the
    dtype has from the record's orient, conv, cent_x (shiftX) and cent_y (shiftY)"""
    p0, p1 = int(p0), int(p1)
    req = np.zeros(max(0, p1 - p0), dtype=dtype)
    req["particle"] = np.arange(p0, p1)
    for f in dtype.names[1:]:
        req[f] = pmap[{"shiftX": "cent_x", "shiftY": "cent_y"}.get(f, f)][p0:p1]
    return req


def _first_or_tuple(first, *extras):
    """first alone, or the tuple of it and the extras that were asked for (those not None)"""
    out = (first,) + tuple(e for e in extras if e is not None)
    return out[0] if len(out) == 1 else out


def ring_count(N):
    """rings of an N x N image (bioem_hip_ring_count): the rounded radius of the corner coefficient plus one; no device"""
    return int(load_library().bioem_hip_ring_count(int(N)))


def window_offsets(N, maxD, grid, algo):
    """the shifts X_0 < X_1 < ... the reference can report for this displacement window (bioem_hip_window_offsets): the
    cell coordinates of a window_posterior table on both axes; int32 [nd].  No device; ValueError on invalid arguments."""
    L = load_library()
    nd = int(L.bioem_hip_window_count(int(N), int(maxD), int(grid), int(algo)))
    if nd <= 0:
        raise ValueError("no displacement window for N %d, maxD %d, grid %d, ALGO %d" % (N, maxD, grid, algo))
    X = np.zeros(nd, dtype=np.int32)
    assert L.bioem_hip_window_offsets(int(N), int(maxD), int(grid), int(algo), _p(X), nd) == nd
    return X


def new_prob_block(nMaps, nAngles, writeAngles):
    """Initialised probability block as run() does (reference bioem.cpp:681-699): returns (raw uint8 array,
    pmap view, pang view or None)."""
    nbytes = nMaps * 40 + (nMaps * nAngles * 16 if writeAngles else 0)
    raw = np.zeros(nbytes, dtype=np.uint8)
    pmap = raw[:nMaps * 40].view(PROB_MAP_DTYPE)
    pmap["Total"] = 0.0
    pmap["Constoadd"] = MIN_PROB
    pang = None
    if writeAngles:
        pang = raw[nMaps * 40:].view(PROB_ANGLE_DTYPE).reshape(nAngles, nMaps)
        pang["forAngles"] = 0.0
        pang["ConstAngle"] = MIN_PROB
    return raw, pmap, pang


class Engine:
    """One GPU's comparison engine; method names mirror the plugin hooks of the reference
    (deviceInit / deviceStartRun / compareRefMaps / deviceFinishRun, include/bioem.h:52-79)."""

    def __init__(self, pd, nMaps, nAngles, nCTF, algo=1, device=0, shard=None):
        """shard = (iOrientBegin, iOrientEnd): bioem_hip_create_shard -- the handle owns that block of the nAngles
        global orientations, keeps its angle table on the device and moves only the map entries in start/finish_run."""
        self.L = load_library()
        self.h = C.c_void_p()
        self.pd = pd
        self.nMaps, self.nAngles, self.nCTF, self.algo = nMaps, nAngles, nCTF, algo
        self.N = pd.NumberPixels
        self.H = self.N // 2 + 1
        self.shard = shard
        if shard is None:
            rc = self.L.bioem_hip_create(C.byref(self.h), device, C.byref(pd), nMaps, nAngles, nCTF, algo)
        else:
            rc = self.L.bioem_hip_create_shard(C.byref(self.h), device, C.byref(pd), nMaps, nAngles, nCTF, algo,
                                               int(shard[0]), int(shard[1]))
        if rc:
            msg = self.L.bioem_hip_last_error(self.h).decode() if self.h else "create failed"
            raise RuntimeError("bioem_hip_create: " + msg)

    def _chk(self, rc, what):
        if rc:
            e = RuntimeError("%s: %s" % (what, self.L.bioem_hip_last_error(self.h).decode()))
            e.rc = rc
            raise e

    def close(self):
        if self.h:
            self.L.bioem_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def fast_path(self):
        return bool(self.L.bioem_hip_uses_fast_path(self.h))

    @property
    def kernel_name(self):
        return self.L.bioem_hip_kernel_name(self.h).decode()

    @property
    def kernel_signature(self):
        return self.L.bioem_hip_kernel_signature(self.h).decode()

    @property
    def own_kernel_signature(self):
        """what compare_own_orientations launches: "k_compare_fast_own<...>" (one launch per batch) or
        "per particle: <kernel_signature>"""
        return self.L.bioem_hip_own_kernel_signature(self.h).decode()

    def set_own_launch(self, mode):
        """how compare_own_orientations launches its comparison: "particle" (one launch per particle, the default),
        "batch" (one launch per batch where the shape has the kernel, bioem_hip_plan_own) or "rows" (the same with the
        block table in plain row order); results do not depend on it"""
        self._chk(self.L.bioem_hip_set_own_launch(self.h, {"particle": 0, "batch": 1, "rows": 2}[mode]), "set_own_launch")

    def set_compare_variant(self, lean):
        """lean (the default of every handle): launches of k_compare_fast that take its static, unsplit 21-row path run the
        lean instantiation of that path; not lean: the full instantiations only.  Same bits either way.  Returns True if
        the launches of this handle now take a lean kernel"""
        return bool(self.L.bioem_hip_set_compare_variant(self.h, 1 if lean else 0))

    def upload_particles(self, refFFT, sumRef, sumsqRef):
        refFFT = np.ascontiguousarray(refFFT, dtype=np.float32)
        assert refFFT.shape == (self.nMaps, self.N, self.H, 2)
        s = np.ascontiguousarray(sumRef, dtype=np.float32)
        s2 = np.ascontiguousarray(sumsqRef, dtype=np.float32)
        self._chk(self.L.bioem_hip_upload_particles(self.h, _p(refFFT), _p(s), _p(s2)), "upload_particles")

    def upload_particle_maps(self, maps):
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        assert maps.shape == (self.nMaps, self.N, self.N)
        self._chk(self.L.bioem_hip_upload_particle_maps(self.h, _p(maps)), "upload_particle_maps")

    def upload_ctf(self, refCTF, ctfParam):
        refCTF = np.ascontiguousarray(refCTF, dtype=np.float32)
        ctfParam = np.ascontiguousarray(ctfParam, dtype=np.float32)
        assert refCTF.shape == (self.nCTF, self.N, self.H, 2) and ctfParam.shape == (self.nCTF, 3)
        self._chk(self.L.bioem_hip_upload_ctf(self.h, _p(refCTF), _p(ctfParam)), "upload_ctf")

    def upload_model(self, points, NormDen, pixelSize, shiftX=0, shiftY=0):
        points = np.ascontiguousarray(points)
        assert points.dtype.itemsize == 24
        self._chk(self.L.bioem_hip_upload_model(self.h, _p(points), len(points), float(NormDen), float(pixelSize),
                                                int(shiftX), int(shiftY)), "upload_model")
        self._nPts = len(points)
        self._volPad = 0

    @staticmethod
    def _centre(centre):
        if centre is None:
            return None
        centre = np.ascontiguousarray(centre, dtype=np.float64)
        assert centre.shape == (3,)
        return centre

    def upload_model_volume(self, vol, pad=2, precorrect=True, centre=None, shiftX=0, shiftY=0):
        """a volume as the model (bioem_hip_upload_model_volume): vol float32 [N, N, N] with its origin at
        voxel (o, o, o), o = (N + 1) // 2, as reconstruct delivers it; replaces a point model.  Projections are then
        central slices of its spectrum on a grid padded by pad (1 or 2), interpolated trilinearly.  precorrect: divide by
        the transform of the trilinear kernel first; centre: float64 [3], the density is moved by -centre pixels
        (volume_model.centre_of_mass); shiftX, shiftY as upload_model.  A refusal raises RuntimeError with .rc == 2 and
        leaves the model as it was."""
        if vol is not None:
            vol = np.ascontiguousarray(vol, dtype=np.float32)
            assert vol.shape == (self.N,) * 3, vol.shape
        centre = self._centre(centre)
        flags = VOLUME_PRECORRECT if precorrect else 0
        self._chk(self.L.bioem_hip_upload_model_volume(self.h, _p(vol), int(pad), flags, _p(centre), int(shiftX),
                                                       int(shiftY)), "upload_model_volume")
        self._nPts = 0
        self._volPad = int(pad)

    def upload_model_spectrum(self, spec, pad=1, centre=None, shiftX=0, shiftY=0):
        """the same from the spectrum itself: spec complex128 [PN, PN, PH], PN = pad N, PH = PN // 2 + 1, un-centred, in
        the layout and sign convention of reconstruct's "spec" at pad = 1 (volume_model.pad_spectrum states it)"""
        if spec is not None:
            spec = np.ascontiguousarray(spec, dtype=np.complex128)
            if pad in (1, 2):
                PN = int(pad) * self.N
                assert spec.shape == (PN, PN, PN // 2 + 1), spec.shape
        centre = self._centre(centre)
        self._chk(self.L.bioem_hip_upload_model_spectrum(self.h, _p(spec), int(pad), _p(centre), int(shiftX), int(shiftY)),
                  "upload_model_spectrum")
        self._nPts = 0
        self._volPad = int(pad)

    def debug_slices(self, angles, isQuat=True):
        """test hook: the slice kernel alone under the orientations angles float32 [n, 4]; complex128 [n, N, H], the
        slices of the volume model as they stand before the rounding to float"""
        angles = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
        out = np.zeros((len(angles), self.N, self.H), dtype=np.complex128)
        self._chk(self.L.bioem_hip_debug_slices(self.h, _p(angles) if len(angles) else None, len(angles), int(bool(isQuat)),
                                                _p(out)), "debug_slices")
        return out

    def upload_orientations(self, angles, isQuat):
        angles = np.ascontiguousarray(angles, dtype=np.float32)
        assert angles.ndim == 2 and angles.shape[1] == 4
        self._chk(self.L.bioem_hip_upload_orientations(self.h, _p(angles), len(angles), int(bool(isQuat))),
                  "upload_orientations")

    def upload_particle_orientations(self, angles, isQuat):
        """one orientation list per particle, angles[nMaps, K, 4] (K <= nAngles): round 2 of the manual's refinement"""
        angles = np.ascontiguousarray(angles, dtype=np.float32)
        assert angles.ndim == 3 and angles.shape[0] == self.nMaps and angles.shape[2] == 4
        self._chk(self.L.bioem_hip_upload_particle_orientations(self.h, _p(angles), angles.shape[1], int(bool(isQuat))),
                  "upload_particle_orientations")

    def upload_particle_orientation_lists(self, lists, isQuat=True):
        """one orientation list per particle, of any length up to nAngles (an empty list leaves the particle out of the
        pass): a sequence of nMaps arrays [K_p, 4], or the tuple (flat [n, 4], offsets [nMaps + 1]), offsets of an integer
        type.  (The two cannot be confused: nMaps + 1 integers are a list of one particle of two only if nMaps is 2, and
        three numbers are no list of quaternions.)"""
        second = np.asarray(lists[1]) if isinstance(lists, tuple) and len(lists) == 2 else None
        if second is not None and second.ndim == 1 and second.dtype.kind in "iu" and len(second) == self.nMaps + 1:
            flat = np.ascontiguousarray(lists[0], dtype=np.float32).reshape(-1, 4)
            offsets = np.ascontiguousarray(lists[1], dtype=np.int64)
        else:
            parts = [np.asarray(a, dtype=np.float32).reshape(-1, 4) for a in lists]
            offsets = np.zeros(len(parts) + 1, dtype=np.int64)
            offsets[1:] = np.cumsum([len(a) for a in parts])
            flat = np.ascontiguousarray(np.concatenate(parts, axis=0)) if parts else np.zeros((0, 4), dtype=np.float32)
        assert len(offsets) == self.nMaps + 1 and (len(offsets) == 0 or offsets[-1] <= len(flat))
        if len(flat) == 0:
            flat = np.zeros((1, 4), dtype=np.float32)  # (a valid pointer; the library refuses the empty total)
        self._chk(self.L.bioem_hip_upload_particle_orientation_lists(self.h, _p(flat), _p(offsets), int(bool(isQuat))),
                  "upload_particle_orientation_lists")

    def prob_bytes(self):
        """bytes start_run / finish_run move: the whole block, or only the map entries for a shard handle"""
        if self.shard is not None:
            return self.L.bioem_hip_prob_size(self.nMaps, 0, 0)
        return self.L.bioem_hip_prob_size(self.nMaps, self.nAngles, self.pd.writeAngles)

    def start_run(self, raw):
        assert raw.nbytes == self.prob_bytes()
        self._chk(self.L.bioem_hip_start_run(self.h, _p(raw)), "start_run")

    def compare(self, iPipeline, iOrient, iConvStart, maxParallelConv, nTotParallelConv, conv_base, params_base):
        """== bioem::compareRefMaps; conv_base [2*nTotParallelConv, N, H, 2], params_base [2*nTotParallelConv]."""
        assert conv_base.dtype == np.float32 and conv_base.flags["C_CONTIGUOUS"]
        assert params_base.dtype == PARAM5_DTYPE and params_base.flags["C_CONTIGUOUS"]
        self._chk(self.L.bioem_hip_compare(self.h, iPipeline, iOrient, iConvStart, maxParallelConv, nTotParallelConv,
                                           _p(conv_base), _p(params_base)), "compare")

    def project_convolve_compare(self, o0, o1):
        self._chk(self.L.bioem_hip_project_convolve_compare(self.h, o0, o1), "project_convolve_compare")

    def project_convolve_compare_ctf(self, o0, o1, c0, c1):
        self._chk(self.L.bioem_hip_project_convolve_compare_ctf(self.h, o0, o1, c0, c1), "project_convolve_compare_ctf")

    def compare_own_orientations(self, p0, p1):
        """particles [p0, p1), each against its own list (upload_particle_orientations) x all CTFs, asynchronous;
        pmap["orient"] is the index in the particle's list"""
        self._chk(self.L.bioem_hip_compare_own_orientations(self.h, p0, p1), "compare_own_orientations")

    def project(self, iPipeline, o0, o1):
        """== bioem::createProjection for [o0, o1), asynchronous; the spectra stay in buffer set iPipeline & 1"""
        self._chk(self.L.bioem_hip_project(self.h, iPipeline, o0, o1), "project")

    def convolve(self, iPipeline, c0, c1):
        """== bioem::createConvolutedProjectionMap for the projections of the set x CTFs [c0, c1), asynchronous"""
        self._chk(self.L.bioem_hip_convolve(self.h, iPipeline, c0, c1), "convolve")

    def compare_device(self, iPipeline):
        """== bioem::compareRefMaps for the conv spectra of the set, asynchronous"""
        self._chk(self.L.bioem_hip_compare_device(self.h, iPipeline), "compare_device")

    def max_batch(self):
        a, b = C.c_int(), C.c_int()
        self._chk(self.L.bioem_hip_max_batch(self.h, C.byref(a), C.byref(b)), "max_batch")
        return a.value, b.value

    def set_phase_timing(self, on):
        self._chk(self.L.bioem_hip_set_phase_timing(self.h, int(bool(on))), "set_phase_timing")

    def phase_records(self):
        """per-batch device time of projection (0) / convolution (1) / comparison (2) since set_phase_timing(True)"""
        n = C.c_int()
        self._chk(self.L.bioem_hip_phase_records(self.h, None, 0, C.byref(n)), "phase_records")
        out = np.zeros(n.value, dtype=PHASE_RECORD_DTYPE)
        if n.value:
            self._chk(self.L.bioem_hip_phase_records(self.h, _p(out), n.value, C.byref(n)), "phase_records")
        return out

    def finish_run(self, raw):
        assert raw.nbytes == self.prob_bytes()
        self._chk(self.L.bioem_hip_finish_run(self.h, _p(raw)), "finish_run")

    def topk_angles(self, K, numconst):
        """K best orientations per particle among the owned ones, selected on the device: [nMaps, K] CANDIDATE_DTYPE.
        The writer's result for a handle that owns the whole list.  The merge of shards' K-wide lists reproduces the
        writer only while no equal keys meet a shard's threshold; merge_candidates gives the lists that always do."""
        out = np.zeros((self.nMaps, K), dtype=CANDIDATE_DTYPE)
        self._chk(self.L.bioem_hip_topk_angles(self.h, K, float(numconst), _p(out)), "topk_angles")
        return out

    def merge_candidates(self, K, numconst):
        """what a shard contributes to a merge: [nMaps, 2K - 1] CANDIDATE_DTYPE, slots 0 ... K-1 = topk_angles, then in
        ascending orientation the entries of the K-th best key that the block's own walk rejected or evicted but a walk
        over the whole list may keep (include/bioem_hip.h); orient = -1 in unused slots.  merge_topk_host(lists, K=K)
        of such lists is the writer's K best of the whole table for any keys and any cut."""
        out = np.zeros((self.nMaps, 2 * K - 1), dtype=CANDIDATE_DTYPE)
        self._chk(self.L.bioem_hip_merge_candidates(self.h, K, float(numconst), _p(out)), "merge_candidates")
        return out

    def debug_topk(self, table, o0, K, W, numconst):
        """test hook: the selection kernel of topk_angles / merge_candidates on a table handed in, PROB_ANGLE_DTYPE
        [nO, nMaps] whose first row is orientation o0; W = K or 2K - 1.  Returns CANDIDATE_DTYPE [nMaps, W]."""
        table = np.ascontiguousarray(table, dtype=PROB_ANGLE_DTYPE)
        nO, nMaps = table.shape
        out = np.zeros((nMaps, W), dtype=CANDIDATE_DTYPE)
        self._chk(self.L.bioem_hip_debug_topk(self.h, _p(table), nO, nMaps, int(o0), int(K), int(W), float(numconst),
                                              _p(out)), "debug_topk")
        return out

    def debug_merge_gathered(self, gathered, nShards, K):
        """test hook: what bioem_hip_merge does after its all-gather, on `gathered` = nShards payloads (uint8; per
        payload nMaps map entries, then with K > 0 nMaps lists of 2K - 1 candidates).  Returns (PROB_MAP_DTYPE [nMaps],
        CANDIDATE_DTYPE [nMaps, K] or None)."""
        gathered = np.ascontiguousarray(gathered, dtype=np.uint8).reshape(-1)
        payload = self.nMaps * (PROB_MAP_DTYPE.itemsize + (CANDIDATE_DTYPE.itemsize * (2 * K - 1) if K > 0 else 0))
        assert gathered.size == nShards * payload
        pmap = np.zeros(self.nMaps, dtype=PROB_MAP_DTYPE)
        cand = np.zeros((self.nMaps, K), dtype=CANDIDATE_DTYPE) if K > 0 else None
        self._chk(self.L.bioem_hip_debug_merge_gathered(self.h, _p(gathered), int(nShards), int(K), _p(pmap), _p(cand)),
                  "debug_merge_gathered")
        return pmap, cand

    def render_best_maps(self, pmap, p0=0, p1=None, own=False):
        """the calculated image of the best match of particles [p0, p1): float32 [p1 - p0, N, N] with
        out[p, (k + X) mod N, (j + Y) mod N] = conv[k, j] / N^2 * norm + mu for the record (orient, conv, X, Y, norm, mu) of
        pmap (PROB_MAP_DTYPE [nMaps], global particle indices: the block of finish_run or a merged one); own: orient
        indexes the particle's own list.  Call outside a run.  A refused record raises RuntimeError with .rc == 2."""
        pmap = _pmap(pmap, self.nMaps)
        p1 = self.nMaps if p1 is None else int(p1)
        out = np.empty((max(0, p1 - int(p0)), self.N, self.N), dtype=np.float32)
        self._chk(self.L.bioem_hip_render_best_maps(self.h, _p(pmap), int(bool(own)), int(p0), p1, _p(out)), "render_best_maps")
        return out

    def best_match_rings(self, pmap, p0=0, p1=None, own=False):
        """per Fourier ring the sums of particles [p0, p1) against the spectrum of their best match: RING_SUMS_DTYPE
        [p1 - p0, ring_count(N)] with cross = sum w Re(R conj(M)), powParticle = sum w |R|^2, powModel = sum w |M|^2 (R the
        particle's spectrum, M the spectrum of the image render_best_maps writes for the record, w the weight of the
        Hermitian partner; include/bioem_hip.h).  pmap, own and the calling rules as render_best_maps; needs the
        particles.  A refused record raises RuntimeError with .rc == 2."""
        pmap = _pmap(pmap, self.nMaps)
        p1 = self.nMaps if p1 is None else int(p1)
        out = np.zeros((max(0, p1 - int(p0)), ring_count(self.N)), dtype=RING_SUMS_DTYPE)
        self._chk(self.L.bioem_hip_best_match_rings(self.h, _p(pmap), int(bool(own)), int(p0), p1, _p(out)), "best_match_rings")
        return out

    def debug_ring_sums(self, specR, specP, records):
        """test hook: the ring kernel of best_match_rings on n spectrum pairs handed in, float32 [n, N, H, 2] each (or
        complex64 [n, N, H]); records: PROB_MAP_DTYPE [n], of which conv, cent_x, cent_y, norm and mu are used.  Needs
        the CTF kernels only.  Returns RING_SUMS_DTYPE [n, ring_count(N)]; a refusal raises with .rc == 2."""
        specR, specP = _spectra(specR), _spectra(specP)
        records = np.ascontiguousarray(records, dtype=PROB_MAP_DTYPE)
        n = len(records)
        assert specR.shape == (n, self.N, self.H, 2) and specP.shape == specR.shape
        out = np.zeros((n, ring_count(self.N)), dtype=RING_SUMS_DTYPE)
        self._chk(self.L.bioem_hip_debug_ring_sums(self.h, _p(specR), _p(specP), _p(records), n, _p(out)), "debug_ring_sums")
        return out

    def _view_args(self, pmap, group_of, weights, n):
        group_of = np.ascontiguousarray(group_of, dtype=np.int32)
        assert group_of.shape == (n,)
        return _pmap(pmap, n), group_of, _vector(weights, n)

    def view_sums(self, pmap, group_of, weights=None, g0=0, g1=None, n_groups=None):
        """the normal equations of the aligned average of every group in [g0, g1) (include/bioem_hip.h): returns
        (num complex128 [g1 - g0, N, H], den float64 [g1 - g0, N, H], stats float64 [g1 - g0, 2] = count, sumw).
        pmap: PROB_MAP_DTYPE [nMaps] (conv, cent_x, cent_y, norm, mu are read); group_of: int [nMaps], -1 = left out;
        weights: float64 [nMaps] >= 0 or None (1); n_groups: max(group_of) + 1 unless given.  Needs the particles and the
        CTF kernels.  A refusal raises RuntimeError with .rc == 2."""
        pmap, group_of, weights = self._view_args(pmap, group_of, weights, self.nMaps)
        nG = int(group_of.max()) + 1 if n_groups is None else int(n_groups)
        g1 = nG if g1 is None else int(g1)
        n = max(0, g1 - int(g0))
        num = np.zeros((n, self.N, self.H), dtype=np.complex128)
        den = np.zeros((n, self.N, self.H), dtype=np.float64)
        stats = np.zeros((n, 2), dtype=np.float64)
        self._chk(self.L.bioem_hip_view_sums(self.h, _p(pmap), _p(weights), _p(group_of), nG, int(g0), g1, _p(num), _p(den),
                                             _p(stats)), "view_sums")
        return num, den, stats

    def view_averages(self, pmap, group_of, group_orient, weights=None, wiener=0.1, g0=0, g1=None, maps=True):
        """the aligned average of every group in [g0, g1) against the projection of its orientation: returns
        (rings RING_SUMS_DTYPE [g1 - g0, ring_count(N)], avg float32 [g1 - g0, N, N], proj likewise); maps=False: rings only
        (avg = proj = None).  group_orient: int [nGroups] into the shared orientation list, -1 = no projection.  P^ = num /
        (den + wiener * mean den); rings: powParticle = power of P^, powModel = power of the projection spectrum."""
        pmap, group_of, weights = self._view_args(pmap, group_of, weights, self.nMaps)
        group_orient = np.ascontiguousarray(group_orient, dtype=np.int32)
        nG = len(group_orient)
        g1 = nG if g1 is None else int(g1)
        n = max(0, g1 - int(g0))
        rings = np.zeros((n, ring_count(self.N)), dtype=RING_SUMS_DTYPE)
        avg = np.zeros((n, self.N, self.N), dtype=np.float32) if maps else None
        proj = np.zeros((n, self.N, self.N), dtype=np.float32) if maps else None
        self._chk(self.L.bioem_hip_view_averages(self.h, _p(pmap), _p(weights), _p(group_of), _p(group_orient), nG,
                                                 float(wiener), int(g0), g1, _p(rings), _p(avg), _p(proj)), "view_averages")
        return rings, avg, proj

    def debug_view_sums(self, specR, pmap, group_of, weights=None, n_groups=None):
        """test hook: the accumulation kernel of view_sums on n spectra handed in, float32 [n, N, H, 2] or complex64
        [n, N, H] in reference layout; pmap, group_of, weights run over the n spectra.  Needs the CTF kernels only.
        Returns (num, den, stats) for all groups as view_sums does."""
        specR = _spectra(specR)
        n = len(specR)
        assert specR.shape == (n, self.N, self.H, 2)
        pmap, group_of, weights = self._view_args(pmap, group_of, weights, n)
        nG = int(group_of.max()) + 1 if n_groups is None else int(n_groups)
        num = np.zeros((max(nG, 0), self.N, self.H), dtype=np.complex128)
        den = np.zeros((max(nG, 0), self.N, self.H), dtype=np.float64)
        stats = np.zeros((max(nG, 0), 2), dtype=np.float64)
        self._chk(self.L.bioem_hip_debug_view_sums(self.h, _p(specR), _p(pmap), _p(weights), _p(group_of), n, nG, _p(num),
                                                   _p(den), _p(stats)), "debug_view_sums")
        return num, den, stats

    def reconstruct(self, pmap, group_of, group_orient, weights=None, wiener=0.1, correct=True, want_spec=False,
                    want_vol=True, cull=True):
        """the 3D density the aligned view sums of the groups support under their orientations (include/bioem_hip.h, DESIGN
        2.20).  Arguments as view_averages; groups with group_orient -1 or no member are skipped.  Returns a dict: "vol"
        float32 [N, N, N] with its origin at voxel (o, o, o), o = (N + 1) // 2 (unless want_vol=False); "stats" float64 [4]
        = views used, particles used, the sum of their weights, tau; with want_spec "spec" complex128 [N, N, H] = V^ and
        "den" float64 [N, N, H] = denV.  correct: divide by the transform of the interpolation kernel; cull=False: the
        test switch BIOEM_HIP_RECON_NO_CULL (same bits).  A refusal raises RuntimeError with .rc == 2."""
        pmap, group_of, weights = self._view_args(pmap, group_of, weights, self.nMaps)
        group_orient = np.ascontiguousarray(group_orient, dtype=np.int32)
        shape = (self.N, self.N, self.H)
        out = {"stats": np.zeros(4, dtype=np.float64)}
        if want_vol:
            out["vol"] = np.zeros((self.N,) * 3, dtype=np.float32)
        if want_spec:
            out["spec"] = np.zeros(shape, dtype=np.complex128)
            out["den"] = np.zeros(shape, dtype=np.float64)
        flags = (RECON_CORRECT if correct else 0) | (0 if cull else RECON_NO_CULL)
        self._chk(self.L.bioem_hip_reconstruct(self.h, _p(pmap), _p(weights), _p(group_of), _p(group_orient),
                                               len(group_orient), float(wiener), flags, _p(out.get("vol")),
                                               _p(out.get("spec")), _p(out.get("den")), _p(out["stats"])), "reconstruct")
        return out

    def debug_reconstruct(self, num, den, angles, isQuat=True, wiener=0.1, correct=True, cull=True, want_vol=True,
                          want_spec=True, want_sums=True, flags=None):
        """test hook: the kernels of reconstruct alone on the sums of n views handed in, num complex128 [n, N, H] and den
        float64 [n, N, H] as view_sums delivers them, under the orientations angles float32 [n, 4].  Needs only the
        handle's parameters.  Returns a dict with "vol" float32 [N, N, N], "spec" complex128 [N, N, H] = V^, "numV"
        complex128 and "denV" float64 [N, N, H], each where asked for; flags overrides correct / cull with raw flag bits.
        A refusal raises with .rc == 2."""
        num = np.ascontiguousarray(num, dtype=np.complex128)
        den = np.ascontiguousarray(den, dtype=np.float64)
        angles = np.ascontiguousarray(angles, dtype=np.float32)
        n = len(angles)
        assert angles.shape == (n, 4) and num.shape == (n, self.N, self.H) and den.shape == num.shape
        shape = (self.N, self.N, self.H)
        out = {}
        if want_vol:
            out["vol"] = np.zeros((self.N,) * 3, dtype=np.float32)
        if want_spec:
            out["spec"] = np.zeros(shape, dtype=np.complex128)
        if want_sums:
            out["numV"] = np.zeros(shape, dtype=np.complex128)
            out["denV"] = np.zeros(shape, dtype=np.float64)
        if flags is None:
            flags = (RECON_CORRECT if correct else 0) | (0 if cull else RECON_NO_CULL)
        self._chk(self.L.bioem_hip_debug_reconstruct(self.h, _p(num) if n else None, _p(den) if n else None,
                                                     _p(angles) if n else None, int(bool(isQuat)), n, float(wiener),
                                                     int(flags), _p(out.get("vol")), _p(out.get("spec")), _p(out.get("numV")),
                                                     _p(out.get("denV"))), "debug_reconstruct")
        return out

    def _soft_args(self, members, cells, shifts):
        members = np.ascontiguousarray(members, dtype=SOFT_MEMBER_DTYPE).reshape(-1)
        shifts = np.ascontiguousarray(self.window_shifts() if shifts is None else shifts, dtype=np.int32).reshape(-1)
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        assert cells.shape == (len(members), len(shifts), len(shifts)), cells.shape
        return members, cells, shifts

    @staticmethod
    def _soft_groups(members, n_groups):
        return (int(members["group"].max()) + 1 if len(members) else 0) if n_groups is None else int(n_groups)

    def view_sums_soft(self, members, cells, shifts=None, g0=0, g1=None, n_groups=None):
        """the normal equations of view_sums under tables of weighted shifts (include/bioem_hip.h): members
        SOFT_MEMBER_DTYPE [n] = one (particle, group, conv) each with its s2, b, mass (group -1 = left out), cells float64
        [n, nd, nd] with cell [i, j] = a at the shift (shifts[i], shifts[j]); shifts: int [nd], window_shifts() unless
        given; n_groups: max group + 1 unless given.  Returns (num, den, stats) for the groups [g0, g1) as view_sums does,
        stats = number of members, sum of mass.  bioem_amd/soft_views.py builds members from a posterior.  A refusal
        raises RuntimeError with .rc == 2."""
        members, cells, shifts = self._soft_args(members, cells, shifts)
        nG = self._soft_groups(members, n_groups)
        g1 = nG if g1 is None else int(g1)
        n = max(0, g1 - int(g0))
        num = np.zeros((n, self.N, self.H), dtype=np.complex128)
        den = np.zeros((n, self.N, self.H), dtype=np.float64)
        stats = np.zeros((n, 2), dtype=np.float64)
        self._chk(self.L.bioem_hip_view_sums_soft(self.h, _p(members), _p(cells), len(members), _p(shifts), len(shifts), nG,
                                                  int(g0), g1, _p(num), _p(den), _p(stats)), "view_sums_soft")
        return num, den, stats

    def debug_view_sums_soft(self, specR, members, cells, shifts=None, n_groups=None):
        """test hook: the kernels of view_sums_soft on spectra handed in, float32 [nSpec, N, H, 2] or complex64 [nSpec, N, H]
        in reference layout; `particle` of a member indexes them.  Needs the CTF kernels only.  Returns (num, den, stats)
        for all groups."""
        specR = _spectra(specR)
        assert specR.shape[1:] == (self.N, self.H, 2)
        members, cells, shifts = self._soft_args(members, cells, shifts)
        nG = self._soft_groups(members, n_groups)
        num = np.zeros((max(nG, 0), self.N, self.H), dtype=np.complex128)
        den = np.zeros((max(nG, 0), self.N, self.H), dtype=np.float64)
        stats = np.zeros((max(nG, 0), 2), dtype=np.float64)
        self._chk(self.L.bioem_hip_debug_view_sums_soft(self.h, _p(specR), len(specR), _p(members), _p(cells), len(members),
                                                        _p(shifts), len(shifts), nG, _p(num), _p(den), _p(stats)),
                  "debug_view_sums_soft")
        return num, den, stats

    def reconstruct_soft(self, members, cells, group_orient, shifts=None, wiener=0.1, correct=True, want_spec=False,
                         want_vol=True, cull=True):
        """reconstruct with the accumulation of view_sums_soft in place of the hard one: members, cells and shifts as
        there, group_orient int [nGroups] into the shared orientation list (-1 = skipped).  Returns the dict of
        reconstruct; "stats" = views used, members used, the sum of their mass, tau."""
        members, cells, shifts = self._soft_args(members, cells, shifts)
        group_orient = np.ascontiguousarray(group_orient, dtype=np.int32)
        shape = (self.N, self.N, self.H)
        out = {"stats": np.zeros(4, dtype=np.float64)}
        if want_vol:
            out["vol"] = np.zeros((self.N,) * 3, dtype=np.float32)
        if want_spec:
            out["spec"] = np.zeros(shape, dtype=np.complex128)
            out["den"] = np.zeros(shape, dtype=np.float64)
        flags = (RECON_CORRECT if correct else 0) | (0 if cull else RECON_NO_CULL)
        self._chk(self.L.bioem_hip_reconstruct_soft(self.h, _p(members), _p(cells), len(members), _p(shifts), len(shifts),
                                                    _p(group_orient), len(group_orient), float(wiener), flags,
                                                    _p(out.get("vol")), _p(out.get("spec")), _p(out.get("den")),
                                                    _p(out["stats"])), "reconstruct_soft")
        return out

    def soft_members(self, pmap, K=1, topk=None, sum_ref=None, own=False, weights=None, log_prior=None, batch=4096,
                     want_weights=False):
        """the members of view_sums_soft / reconstruct_soft from the posterior of a finished run (bioem_amd/soft_views.py):
        K = 1: every CTF set and every window cell at the arg-max orientation of each particle of pmap (PROB_MAP_DTYPE
        [nMaps]); K >= 2: at the first K orientations of topk (CANDIDATE_DTYPE [nMaps, >= K], topk_angles or a merged
        ranking).  group = orientation.  window_posterior runs over the requests `batch` at a time.  sum_ref: the
        particles' sums float32 [nMaps] (debug_particles unless given); weights: float64 [nMaps] or None; log_prior:
        float64 [nAngles] or None.  Returns (members, cells, requests), with want_weights the posterior weights float64
        [n, nd, nd] as well."""
        from . import soft_views
        pmap = _pmap(pmap, self.nMaps)
        if int(K) <= 1:
            req, group = soft_views.requests_best(pmap, self.nCTF)
        else:
            if topk is None:
                raise ValueError("soft_members: K >= 2 needs the candidates of topk_angles")
            req, group = soft_views.requests_topk(topk, int(K), self.nCTF)
        nd = len(self.window_shifts())
        logp = np.zeros((len(req), nd, nd), dtype=np.float64)
        cc = np.zeros((len(req), nd, nd), dtype=np.float32)
        par = np.zeros(len(req), dtype=PARAM5_DTYPE)
        for i0 in range(0, len(req), int(batch)):
            i1 = min(len(req), i0 + int(batch))
            logp[i0:i1], cc[i0:i1], par[i0:i1] = self.window_posterior(req[i0:i1], own=own, want_cc=True, want_params=True)
        if sum_ref is None:
            sum_ref = self.debug_particles()[1]
        out = soft_views.members(req, group, logp, cc, par, sum_ref, self.N, weights=weights, log_prior=log_prior,
                                 want_weights=want_weights)
        return out[:2] + (req,) + out[2:]

    def window_shifts(self):
        """the cell coordinates of this handle's window tables (window_offsets of its parameters)"""
        return window_offsets(self.N, self.pd.maxDisplaceCenter, self.pd.GridSpaceCenter, self.algo)

    def window_posterior(self, requests, own=False, want_cc=False, want_params=False):
        """the log posterior of every cell of the displacement window for each request (particle, orient, conv) of
        WINDOW_REQUEST_DTYPE [n] (or an [n, 3] integer array): float64 [n, nd, nd], cell [i, j] at the reported shift
        (X_i, X_j) of window_shifts() (include/bioem_hip.h).  orient indexes the shared list, with own=True the list of
        the request's particle.  Requests are independent and may repeat particles in any order.  want_cc adds the
        float32 cross-correlation values [n, nd, nd], want_params the PARAM5_DTYPE [n] of the requests' (orient, conv)
        pairs; the result is then a tuple in that order.  Outside a run; a refusal raises RuntimeError with .rc == 2."""
        r = _requests(requests, WINDOW_REQUEST_DTYPE)
        n, nd = len(r), len(self.window_shifts())
        logp = np.zeros((n, nd, nd), dtype=np.float64)
        cc = np.zeros((n, nd, nd), dtype=np.float32) if want_cc else None
        par = np.zeros(n, dtype=PARAM5_DTYPE) if want_params else None
        self._chk(self.L.bioem_hip_window_posterior(self.h, _p(r) if n else None, n, int(bool(own)), _p(logp), _p(cc), _p(par)),
                  "window_posterior")
        return _first_or_tuple(logp, cc, par)

    def best_match_window(self, pmap, p0=0, p1=None, own=False, want_cc=False, want_params=False):
        """window_posterior of the best record (orient, conv) of particles [p0, p1) of a probability block's map
        entries (PROB_MAP_DTYPE [nMaps]); own as for render_best_maps"""
        req = _match_requests(_pmap(pmap, self.nMaps), p0, self.nMaps if p1 is None else p1, WINDOW_REQUEST_DTYPE)
        return self.window_posterior(req, own=own, want_cc=want_cc, want_params=want_params)

    def debug_window(self, specConv, specRef, params, sumRef, sumsqRef):
        """test hook: the window kernels of window_posterior on n spectrum pairs handed in, float32 [n, N, H, 2] each (or
        complex64 [n, N, H]), with params PARAM5_DTYPE [n] and the particles' sums float32 [n].  Needs only the handle's
        parameters.  Returns (logp float64 [n, nd, nd], cc float32 [n, nd, nd]); a refusal raises with .rc == 2."""
        specConv, specRef = _spectra(specConv), _spectra(specRef)
        params = np.ascontiguousarray(params, dtype=PARAM5_DTYPE)
        n, nd = len(params), len(self.window_shifts())
        sumRef = np.ascontiguousarray(sumRef, dtype=np.float32)
        sumsqRef = np.ascontiguousarray(sumsqRef, dtype=np.float32)
        assert specConv.shape == (n, self.N, self.H, 2) and specRef.shape == specConv.shape
        assert sumRef.shape == (n,) and sumsqRef.shape == (n,)
        logp = np.zeros((n, nd, nd), dtype=np.float64)
        cc = np.zeros((n, nd, nd), dtype=np.float32)
        self._chk(self.L.bioem_hip_debug_window(self.h, _p(specConv), _p(specRef), _p(params), _p(sumRef), _p(sumsqRef), n,
                                                _p(logp), _p(cc)), "debug_window")
        return logp, cc

    def _scan_candidates(self, kernels, ctf_params):
        kernels = _spectra(kernels)
        ctf_params = np.ascontiguousarray(ctf_params, dtype=np.float32)
        assert kernels.ndim == 4 and kernels.shape[1:] == (self.N, self.H, 2), kernels.shape
        assert ctf_params.shape == (len(kernels), 3), ctf_params.shape
        return kernels, ctf_params

    def ctf_scan(self, requests, kernels, ctf_params, own=False, want_cc=False, want_params=False):
        """the log posterior of each request (particle, orient, shiftX, shiftY) of SCAN_REQUEST_DTYPE [n] (or an [n, 4]
        integer array) under every candidate CTF set: kernels float32 [G, N, H, 2] (or complex64 [G, N, H]) in the layout
        upload_ctf takes, ctf_params float32 [G, 3] = (amp, phase, env).  Returns float64 [n, G]: entry [r, g] is the cell
        (shiftX, shiftY) of the window_posterior table had candidate g been a CTF set of the handle (include/bioem_hip.h);
        a shift need not be a cell of the handle's window, |shift| < N.  orient indexes the shared list, with own=True the
        list of the request's particle.  want_cc adds the float32 cross-correlation values [n, G], want_params the
        PARAM5_DTYPE [n, G] of the (request, candidate) pairs; the result is then a tuple in that order.  Outside a run;
        a refusal raises RuntimeError with .rc == 2."""
        r = _requests(requests, SCAN_REQUEST_DTYPE)
        kernels, ctf_params = self._scan_candidates(kernels, ctf_params)
        n, G = len(r), len(kernels)
        logp = np.zeros((n, G), dtype=np.float64)
        cc = np.zeros((n, G), dtype=np.float32) if want_cc else None
        par = np.zeros((n, G), dtype=PARAM5_DTYPE) if want_params else None
        self._chk(self.L.bioem_hip_ctf_scan(self.h, _p(r) if n else None, n, int(bool(own)), _p(kernels) if G else None,
                                            _p(ctf_params) if G else None, G, _p(logp), _p(cc), _p(par)), "ctf_scan")
        return _first_or_tuple(logp, cc, par)

    def best_match_ctf_scan(self, pmap, kernels, ctf_params, p0=0, p1=None, own=False, want_cc=False, want_params=False):
        """ctf_scan of the best record (orient, cent_x, cent_y) of particles [p0, p1) of a probability block's map entries
        (PROB_MAP_DTYPE [nMaps]); own as for render_best_maps"""
        req = _match_requests(_pmap(pmap, self.nMaps), p0, self.nMaps if p1 is None else p1, SCAN_REQUEST_DTYPE)
        return self.ctf_scan(req, kernels, ctf_params, own=own, want_cc=want_cc, want_params=want_params)

    def debug_ctf_scan(self, specP, specRef, sumRef, sumsqRef, shifts, kernels, ctf_params):
        """test hook: the kernels of ctf_scan on n (projection, particle) spectrum pairs handed in, float32 [n, N, H, 2] each
        (or complex64 [n, N, H]), with the particles' sums float32 [n] and the shifts int [n, 2].  Needs only the handle's
        parameters.  Returns (logp float64 [n, G], cc float32 [n, G], params PARAM5_DTYPE [n, G]); a refusal raises with
        .rc == 2."""
        specP, specRef = _spectra(specP), _spectra(specRef)
        kernels, ctf_params = self._scan_candidates(kernels, ctf_params)
        n, G = len(specP), len(kernels)
        sumRef = np.ascontiguousarray(sumRef, dtype=np.float32)
        sumsqRef = np.ascontiguousarray(sumsqRef, dtype=np.float32)
        shifts = np.ascontiguousarray(shifts, dtype=np.int32)
        assert specP.shape == (n, self.N, self.H, 2) and specRef.shape == specP.shape
        assert sumRef.shape == (n,) and sumsqRef.shape == (n,) and shifts.shape == (n, 2)
        logp = np.zeros((n, G), dtype=np.float64)
        cc = np.zeros((n, G), dtype=np.float32)
        par = np.zeros((n, G), dtype=PARAM5_DTYPE)
        self._chk(self.L.bioem_hip_debug_ctf_scan(self.h, _p(specP), _p(specRef), _p(sumRef), _p(sumsqRef), _p(shifts), n,
                                                  _p(kernels) if G else None, _p(ctf_params) if G else None, G, _p(logp),
                                                  _p(cc), _p(par)), "debug_ctf_scan")
        return logp, cc, par

    def model_gradient(self, requests, weights=None, own=False, want_grad=True, want_params=False):
        """the derivative of the log posterior of each request (particle, orient, conv, shiftX, shiftY) of
        GRAD_REQUEST_DTYPE [n] (or an [n, 5] integer array) with respect to the density of every model point
        (include/bioem_hip.h).  Returns a dict: "points" GRAD_POINT_DTYPE [nPts], the sums over the requests
        in request order with the weights float64 [n] (None: all 1); "coef" float64 [n, 4] = (a, b, g, m); with want_grad
        "grad" float64 [n, nPts]; with want_params "params" PARAM5_DTYPE [n], the linearisation point.  orient indexes the
        shared list, with own=True the list of the request's particle.  Outside a run; a refusal raises RuntimeError
        with .rc == 2."""
        r = _requests(requests, GRAD_REQUEST_DTYPE)
        n, nPts = len(r), getattr(self, "_nPts", 0)   # (no model: the entry refuses)
        w = _vector(weights, n)
        out = {"points": np.zeros(nPts, dtype=GRAD_POINT_DTYPE), "coef": np.zeros((n, 4), dtype=np.float64)}
        if want_grad:
            out["grad"] = np.zeros((n, nPts), dtype=np.float64)
        if want_params:
            out["params"] = np.zeros(n, dtype=PARAM5_DTYPE)
        self._chk(self.L.bioem_hip_model_gradient(self.h, _p(r) if n else None, _p(w), n, int(bool(own)), _p(out.get("grad")),
                                                  _p(out["points"]), _p(out.get("params")), _p(out["coef"])), "model_gradient")
        return out

    def best_match_gradient(self, pmap, p0=0, p1=None, own=False, weights=None, want_grad=True, want_params=False):
        """model_gradient of the best record (orient, conv, cent_x, cent_y) of particles [p0, p1) of a probability block's
        map entries (PROB_MAP_DTYPE [nMaps]); own as for render_best_maps"""
        req = _match_requests(_pmap(pmap, self.nMaps), p0, self.nMaps if p1 is None else p1, GRAD_REQUEST_DTYPE)
        return self.model_gradient(req, weights=weights, own=own, want_grad=want_grad, want_params=want_params)

    def _vol_spec_shape(self):
        PN = max(1, getattr(self, "_volPad", 0)) * self.N   # (no volume model: the entries refuse)
        return (PN, PN, PN // 2 + 1)

    def volume_gradient(self, requests, weights=None, own=False, want_vol=True, want_spec=False, want_params=False):
        """the derivative of the log posterior of the requests (particle, orient, conv, shiftX, shiftY) of
        GRAD_REQUEST_DTYPE [n] (or an [n, 5] integer array), weighted by weights float64 [n] (None: all 1) and summed in
        request order, with respect to every voxel of the volume model (include/bioem_hip.h).  Returns a
        dict: "coef" float64 [n, 4] = (a, b, g, <C, A_r>); "stats" float64 [3] = (n, sum of the weights, requests whose
        coefficients are not finite); with want_vol "vol" float64 [N, N, N], the gradient with respect to the array
        handed to upload_model_volume; with want_spec "spec" complex128 [PN, PN, PH], the gradient A with respect to the
        centred spectrum; with want_params "params" PARAM5_DTYPE [n].  Outside a run; a refusal raises RuntimeError with
        .rc == 2."""
        r = _requests(requests, GRAD_REQUEST_DTYPE)
        n = len(r)
        w = _vector(weights, n)
        out = {"coef": np.zeros((n, 4), dtype=np.float64), "stats": np.zeros(3, dtype=np.float64)}
        if want_vol:
            out["vol"] = np.zeros((self.N,) * 3, dtype=np.float64)
        if want_spec:
            out["spec"] = np.zeros(self._vol_spec_shape(), dtype=np.complex128)
        if want_params:
            out["params"] = np.zeros(n, dtype=PARAM5_DTYPE)
        self._chk(self.L.bioem_hip_volume_gradient(self.h, _p(r) if n else None, _p(w), n, int(bool(own)), _p(out.get("vol")),
                                                   _p(out.get("spec")), _p(out["coef"]), _p(out.get("params")),
                                                   _p(out["stats"])), "volume_gradient")
        return out

    def best_match_volume_gradient(self, pmap, p0=0, p1=None, own=False, weights=None, want_vol=True, want_spec=False,
                                   want_params=False):
        """volume_gradient of the best record (orient, conv, cent_x, cent_y) of particles [p0, p1) of a probability block's
        map entries (PROB_MAP_DTYPE [nMaps]); own as for render_best_maps"""
        req = _match_requests(_pmap(pmap, self.nMaps), p0, self.nMaps if p1 is None else p1, GRAD_REQUEST_DTYPE)
        return self.volume_gradient(req, weights=weights, own=own, want_vol=want_vol, want_spec=want_spec,
                                    want_params=want_params)

    def debug_volume_backproject(self, angles, gamma, weights=None, isQuat=True, cull=True):
        """test hook: Y and the back-insertion alone, on the spectra gamma complex128 [n, N, H] handed in as Gamma under the
        orientations angles float32 [n, 4], scaled by weights float64 [n] alone; complex128 [PN, PN, PH] = A"""
        angles = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
        n = len(angles)
        gamma = np.ascontiguousarray(gamma, dtype=np.complex128)
        assert gamma.shape == (n, self.N, self.H), gamma.shape
        w = _vector(weights, n)
        out = np.zeros(self._vol_spec_shape(), dtype=np.complex128)
        self._chk(self.L.bioem_hip_debug_volume_backproject(self.h, _p(angles) if n else None, n, int(bool(isQuat)),
                                                            _p(gamma) if n else None, _p(w), int(bool(cull)), _p(out)),
                  "debug_volume_backproject")
        return out

    def pose_gradient(self, requests, own=False, want_params=False):
        """the derivative of the log posterior of each request (particle, orient, conv, shiftX, shiftY) of
        GRAD_REQUEST_DTYPE [n] (or an [n, 5] integer array) with respect to rows 0 and 1 of its orientation matrix and to
        the handle's model shifts, for a volume model (include/bioem_hip.h).  Returns a dict: "pose"
        POSE_GRAD_DTYPE [n]; "coef" float64 [n, 4] = (a, b, g, <C, A_r>); with want_params "params" PARAM5_DTYPE [n].
        Outside a run; a refusal raises RuntimeError with .rc == 2."""
        r = _requests(requests, GRAD_REQUEST_DTYPE)
        n = len(r)
        out = {"pose": np.zeros(n, dtype=POSE_GRAD_DTYPE), "coef": np.zeros((n, 4), dtype=np.float64)}
        if want_params:
            out["params"] = np.zeros(n, dtype=PARAM5_DTYPE)
        self._chk(self.L.bioem_hip_pose_gradient(self.h, _p(r) if n else None, n, int(bool(own)), _p(out["pose"]),
                                                 _p(out["coef"]), _p(out.get("params"))), "pose_gradient")
        return out

    def best_match_pose_gradient(self, pmap, p0=0, p1=None, own=False):
        """pose_gradient of the best record (orient, conv, cent_x, cent_y) of particles [p0, p1) of a probability block's
        map entries (PROB_MAP_DTYPE [nMaps]); own as for render_best_maps"""
        req = _match_requests(_pmap(pmap, self.nMaps), p0, self.nMaps if p1 is None else p1, GRAD_REQUEST_DTYPE)
        return self.pose_gradient(req, own=own)

    def debug_pose_sums(self, angles, gamma, weights=None, isQuat=True):
        """test hook: Y and the two pose kernels alone, on the spectra gamma complex128 [n, N, H] handed in as Gamma under
        the orientations angles float32 [n, 4], scaled by weights float64 [n] alone; POSE_GRAD_DTYPE [n]"""
        angles = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
        n = len(angles)
        gamma = np.ascontiguousarray(gamma, dtype=np.complex128)
        assert gamma.shape == (n, self.N, self.H), gamma.shape
        w = _vector(weights, n)
        out = np.zeros(n, dtype=POSE_GRAD_DTYPE)
        self._chk(self.L.bioem_hip_debug_pose_sums(self.h, _p(angles) if n else None, n, int(bool(isQuat)),
                                                   _p(gamma) if n else None, _p(w), _p(out)), "debug_pose_sums")
        return out

    def ctf_gradient(self, requests, pixel_size, own=False, want_params=False):
        """gradient and Hessian of the log posterior of each request (particle, orient, conv, shiftX, shiftY) of
        GRAD_REQUEST_DTYPE [n] (or an [n, 5] integer array) with respect to the triple (amp, pha, env) of its CTF set, at
        the pixel size the kernels were made with (include/bioem_hip.h); CTF mode, point and volume models.
        Returns a dict: "rows" CTF_GRAD_DTYPE [n]; "coef" float64 [n, 4] = (a, b, g, 0); with want_params "params"
        PARAM5_DTYPE [n].  Outside a run; a refusal raises RuntimeError with .rc == 2."""
        r = _requests(requests, GRAD_REQUEST_DTYPE)
        n = len(r)
        out = {"rows": np.zeros(n, dtype=CTF_GRAD_DTYPE), "coef": np.zeros((n, 4), dtype=np.float64)}
        if want_params:
            out["params"] = np.zeros(n, dtype=PARAM5_DTYPE)
        self._chk(self.L.bioem_hip_ctf_gradient(self.h, _p(r) if n else None, n, int(bool(own)), float(pixel_size),
                                                _p(out["rows"]), _p(out["coef"]), _p(out.get("params"))), "ctf_gradient")
        return out

    def best_match_ctf_gradient(self, pmap, pixel_size, p0=0, p1=None, own=False):
        """ctf_gradient of the best record (orient, conv, cent_x, cent_y) of particles [p0, p1) of a probability block's
        map entries (PROB_MAP_DTYPE [nMaps]); own as for render_best_maps"""
        req = _match_requests(_pmap(pmap, self.nMaps), p0, self.nMaps if p1 is None else p1, GRAD_REQUEST_DTYPE)
        return self.ctf_gradient(req, pixel_size, own=own)

    def debug_ctf_gradient(self, specP, specRef, shifts, triples, pixel_size, want_derivs=False):
        """test hook: the three kernels of ctf_gradient on n (projection, particle) spectrum pairs handed in, float32
        [n, N, H, 2] each (or complex64 [n, N, H]), the shifts int [n, 2] and a triple (amp, pha, env) float32 [n, 3] per
        record; a row is finished at the linearisation point its spectra imply (include/bioem_hip.h).  Needs only the
        handle's parameters.  Returns CTF_GRAD_DTYPE [n], with want_derivs also float64 [n, N H, 10]: k, its three first
        and six second derivatives per position of the walk order; a refusal raises with .rc == 2."""
        specP, specRef = _spectra(specP), _spectra(specRef)
        n = len(specP)
        shifts = np.ascontiguousarray(shifts, dtype=np.int32)
        triples = np.ascontiguousarray(triples, dtype=np.float32)
        assert specP.shape == (n, self.N, self.H, 2) and specRef.shape == specP.shape
        assert shifts.shape == (n, 2) and triples.shape == (n, 3)
        rows = np.zeros(n, dtype=CTF_GRAD_DTYPE)
        derivs = np.zeros((n, self.N * self.H, 10), dtype=np.float64) if want_derivs else None
        self._chk(self.L.bioem_hip_debug_ctf_gradient(self.h, _p(specP) if n else None, _p(specRef) if n else None,
                                                      _p(shifts), _p(triples), n, float(pixel_size), _p(rows), _p(derivs)),
                  "debug_ctf_gradient")
        return (rows, derivs) if want_derivs else rows

    def debug_volume_adjoint(self, spec):
        """test hook: the passes from A complex128 [PN, PN, PH] back to the volume alone; float64 [N, N, N]"""
        spec = np.ascontiguousarray(spec, dtype=np.complex128)
        assert spec.shape == self._vol_spec_shape(), spec.shape
        out = np.zeros((self.N,) * 3, dtype=np.float64)
        self._chk(self.L.bioem_hip_debug_volume_adjoint(self.h, _p(spec), _p(out)), "debug_volume_adjoint")
        return out

    def debug_grad_image(self, specConv, specRef, kernels, params, sumRef, sumsqRef, shifts):
        """test hook: a, b, g and the gradient image G_P of n records from conv spectra, particle spectra and kernels handed
        in, float32 [n, N, H, 2] each (or complex64 [n, N, H]), params PARAM5_DTYPE [n], the particles' sums float32 [n]
        and the shifts int [n, 2].  Needs only the handle's parameters.  Returns (gmap float64 [n, N, N], coef float64
        [n, 3]); a refusal raises with .rc == 2."""
        specConv, specRef, kernels = _spectra(specConv), _spectra(specRef), _spectra(kernels)
        n = len(specConv)
        params = np.ascontiguousarray(params, dtype=PARAM5_DTYPE)
        sumRef = np.ascontiguousarray(sumRef, dtype=np.float32)
        sumsqRef = np.ascontiguousarray(sumsqRef, dtype=np.float32)
        shifts = np.ascontiguousarray(shifts, dtype=np.int32)
        assert specConv.shape == (n, self.N, self.H, 2) and specRef.shape == specConv.shape and kernels.shape == specConv.shape
        assert params.shape == (n,) and sumRef.shape == (n,) and sumsqRef.shape == (n,) and shifts.shape == (n, 2)
        gmap = np.zeros((n, self.N, self.N), dtype=np.float64)
        coef = np.zeros((n, 3), dtype=np.float64)
        self._chk(self.L.bioem_hip_debug_grad_image(self.h, _p(specConv), _p(specRef), _p(kernels), _p(params), _p(sumRef),
                                                    _p(sumsqRef), _p(shifts), n, _p(gmap), _p(coef)), "debug_grad_image")
        return gmap, coef

    def debug_grad_gather(self, gmaps, o0=0):
        """test hook: u_k of every model point from the maps float64 [nO, N, N] at the orientations [o0, o0 + nO) of the
        shared list.  Returns float64 [nO, nPts]; a refusal raises with .rc == 2."""
        gmaps = np.ascontiguousarray(gmaps, dtype=np.float64)
        assert gmaps.ndim == 3 and gmaps.shape[1:] == (self.N, self.N), gmaps.shape
        u = np.zeros((len(gmaps), self._nPts), dtype=np.float64)
        self._chk(self.L.bioem_hip_debug_grad_gather(self.h, _p(gmaps), int(o0), len(gmaps), _p(u)), "debug_grad_gather")
        return u

    def orientation_sums(self, prior=None, p0=0, p1=None, own=False):
        """the orientation posterior of particles [p0, p1) reduced where the angle table lives: ORIENT_SUMS_DTYPE
        [p1 - p0] with m = max l, omax (global index; with own lists the index in the particle's list), count, hasMoments
        and the sums S0, S1, S2, Q relative to m, over the entries with forAngles > 0 and l = log forAngles + ConstAngle +
        prior (include/bioem_hip.h; orient_stats.derive turns them into entropy, nEff, mean orientation and spread).
        prior: None, or nAngles log priors by global orientation index (not with own lists).  Call after finish_run on a
        handle with WRITE_PROB_ANGLES; a shard sums over its own block.  A refusal raises RuntimeError with .rc == 2."""
        p1 = self.nMaps if p1 is None else int(p1)
        prior = _vector(prior, self.nAngles)
        out = np.zeros(max(0, p1 - int(p0)), dtype=ORIENT_SUMS_DTYPE)
        self._chk(self.L.bioem_hip_orientation_sums(self.h, _p(prior), int(p0), p1, int(bool(own)), _p(out)), "orientation_sums")
        return out

    def debug_orient_sums(self, table, angles=None, isQuat=True, prior=None, offsets=None):
        """test hook: the kernels of orientation_sums on a table handed in, PROB_ANGLE_DTYPE [nO, nMaps]; angles float32
        [nO, 4] or None (no moments), prior float64 [nO] or None.  offsets (int64 [nMaps + 1]): the own-list instantiation,
        angles = the flat lists.  Returns ORIENT_SUMS_DTYPE [nMaps]; a refusal raises with .rc == 2."""
        table = np.ascontiguousarray(table, dtype=PROB_ANGLE_DTYPE)
        nO, nMaps = table.shape
        if angles is not None:
            angles = np.ascontiguousarray(angles, dtype=np.float32).reshape(-1, 4)
        out = np.zeros(nMaps, dtype=ORIENT_SUMS_DTYPE)
        if offsets is None:
            assert angles is None or len(angles) == nO
            rc = self.L.bioem_hip_debug_orient_sums(self.h, _p(table), nO, nMaps, _p(angles), int(bool(isQuat)),
                                                    _p(_vector(prior, nO)), _p(out))
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            assert offsets.shape == (nMaps + 1,) and prior is None and angles is not None and len(angles) >= offsets[-1]
            rc = self.L.bioem_hip_debug_orient_sums_own(self.h, _p(table), nO, nMaps, _p(angles), _p(offsets),
                                                        int(bool(isQuat)), _p(out))
        self._chk(rc, "debug_orient_sums")
        return out

    def orientation_occupancy(self, sums, prior=None, p0=0, p1=None):
        """the angle table reduced along the particles [p0, p1): ORIENT_OCC_DTYPE [orientations the handle owns] with
        occ = sum_p w, occ2 = sum_p w^2, wmax, pmax (lowest particle index attaining it, -1 for an empty row), count and
        hard (particles whose arg-max is this orientation), w(o, p) = e^(l - m_p) / S0_p the posterior of orientation o for
        particle p (include/bioem_hip.h).  sums: ORIENT_SUMS_DTYPE [p1 - p0], the particles' orientation sums under the
        same prior -- for shards the merged ones (merge_orient_sums).  prior: None, or nAngles log priors by global index.
        Call after finish_run on a handle with WRITE_PROB_ANGLES; a shard returns its block, merge_orient_occupancy
        concatenates them.  A refusal raises RuntimeError with .rc == 2."""
        p1 = self.nMaps if p1 is None else int(p1)
        sums = np.ascontiguousarray(sums, dtype=ORIENT_SUMS_DTYPE)
        assert sums.ndim == 1
        if 0 <= int(p0) < p1 <= self.nMaps:              # (a range the entry refuses reads no sums)
            assert len(sums) == p1 - int(p0)
        prior = _vector(prior, self.nAngles)
        o0, o1 = self.shard if self.shard is not None else (0, self.nAngles)
        out = np.zeros(o1 - o0, dtype=ORIENT_OCC_DTYPE)
        self._chk(self.L.bioem_hip_orientation_occupancy(self.h, _p(prior), _p(sums) if sums.size else None, int(p0), p1,
                                                         _p(out)), "orientation_occupancy")
        return out

    def debug_orient_occupancy(self, table, sums, prior=None, p0=0, p1=None, o0=0):
        """test hook: the kernel of orientation_occupancy on a table handed in, PROB_ANGLE_DTYPE [nO, nMaps]; sums
        ORIENT_SUMS_DTYPE [p1 - p0] for the particles [p0, p1); prior float64 [nO] by row or None; o0 the global index of
        row 0.  Returns ORIENT_OCC_DTYPE [nO]; a refusal raises with .rc == 2."""
        table = np.ascontiguousarray(table, dtype=PROB_ANGLE_DTYPE)
        nO, nMaps = table.shape
        p1 = nMaps if p1 is None else int(p1)
        sums = np.ascontiguousarray(sums, dtype=ORIENT_SUMS_DTYPE)
        assert sums.shape == (p1 - int(p0),)
        prior = _vector(prior, nO)
        out = np.zeros(nO, dtype=ORIENT_OCC_DTYPE)
        self._chk(self.L.bioem_hip_debug_orient_occupancy(self.h, _p(table), nO, nMaps, _p(prior), _p(sums), int(p0), p1,
                                                          int(o0), _p(out)), "debug_orient_occupancy")
        return out

    def enable_ctf_table(self, on=True):
        """keep the posterior per (CTF set, particle) beside the particle entries, from the next start_run on; call it
        outside a run (inside one it raises, .rc == 2)"""
        self._chk(self.L.bioem_hip_enable_ctf_table(self.h, int(bool(on))), "enable_ctf_table")

    def ctf_table(self):
        """[nCTF, nMaps] PROB_MAP_DTYPE: entry (c, p) is what particle p's entry would be had the run compared CTF set c
        only (conv == c; orient / cent_x / cent_y / norm / mu of the best match under that CTF set).  Flushes and
        synchronises.  Without enable_ctf_table it raises with .rc == 2."""
        out = np.zeros((self.nCTF, self.nMaps), dtype=PROB_MAP_DTYPE)
        self._chk(self.L.bioem_hip_ctf_table(self.h, _p(out)), "ctf_table")
        return out

    def synchronize(self):
        self._chk(self.L.bioem_hip_synchronize(self.h), "synchronize")

    def debug_projection(self, iOrient):
        out = np.empty((self.N, self.H, 2), dtype=np.float32)
        self._chk(self.L.bioem_hip_debug_projection(self.h, iOrient, _p(out)), "debug_projection")
        return out

    PROJECTION_PATHS = {"auto": 0, "box": 1, "bands": 2, "atomics": 3}

    def debug_projection_maps(self, o0, nO, path="auto", want_spec=False):
        """the real-space projections of orientations [o0, o0 + nO) of the shared list (bioem_hip_debug_projection_maps;
        nO <= max_batch()[0]): (maps float64 [nO, N, N], tempden float64 [nO], spec float32 [nO, N, H, 2] or None,
        info).  path: "auto" (what a run takes), "box", "bands", "atomics" or 0...3; info: dict path / boxLo / boxSide /
        compact / TR / iradMax.  A forced path the model, list or size does not allow raises with .rc == 2; the handle
        stays usable."""
        nO = int(nO)
        maps = np.zeros((max(nO, 0), self.N, self.N), dtype=np.float64)
        td = np.zeros(max(nO, 0), dtype=np.float64)
        spec = np.zeros((max(nO, 0), self.N, self.H, 2), dtype=np.float32) if want_spec else None
        info = np.zeros(6, dtype=np.int32)
        self._chk(self.L.bioem_hip_debug_projection_maps(self.h, int(o0), nO, int(self.PROJECTION_PATHS.get(path, path)),
                                                         _p(maps), _p(td), _p(spec), _p(info)), "debug_projection_maps")
        return maps, td, spec, dict(zip(("path", "boxLo", "boxSide", "compact", "TR", "iradMax"), map(int, info)))

    def debug_stamps(self):
        """the footprint table of the uploaded model (bioem_hip_debug_stamps): (stamps float64 [nPts, S, S], iradMax),
        S = 2 iradMax + 1; raises with .rc == 2 where the model has none"""
        irad = C.c_int()
        self._chk(self.L.bioem_hip_debug_stamps(self.h, None, C.byref(irad)), "debug_stamps")
        S = 2 * irad.value + 1
        out = np.zeros((self._nPts, S, S), dtype=np.float64)
        self._chk(self.L.bioem_hip_debug_stamps(self.h, _p(out), C.byref(irad)), "debug_stamps")
        return out, irad.value

    def debug_convolution(self, iOrient, iConv):
        out = np.empty((self.N, self.H, 2), dtype=np.float32)
        s, s2 = C.c_float(), C.c_float()
        self._chk(self.L.bioem_hip_debug_convolution(self.h, iOrient, iConv, _p(out), C.byref(s), C.byref(s2)),
                  "debug_convolution")
        return out, np.float32(s.value), np.float32(s2.value)

    def debug_convolve_batch(self, specP, c0, nC, want_raw=False):
        """one convolution batch as a run launches it (bioem_hip_debug_convolve_batch), from the projection spectra specP
        float32 [nO, N, H, 2] and the handle's CTF sets [c0, c0 + nC): (conv float32 [nO nC + 1, N, H, 2] in reference
        layout, params PARAM5_DTYPE [nO nC + 1], raw float32 [nO nC, N Hp, 2] or None, info).  The last conv row and the
        last params entry are the guard: 0xFF bytes no kernel may have touched.  info: dict fused / fast / N1 / Hp / rows /
        guard.  BIOEM_CONVOLVE_FUSED is read at the call.  Invalid arguments raise with .rc == 2; the handle stays usable."""
        specP = _spectra(specP)
        assert specP.ndim == 4 and specP.shape[1:] == (self.N, self.H, 2), specP.shape
        nO, c0, nC = len(specP), int(c0), int(nC)
        rows = max(nO * nC, 0)
        conv = np.zeros((rows + 1, self.N, self.H, 2), dtype=np.float32)
        params = np.zeros(rows + 1, dtype=PARAM5_DTYPE)
        info = np.zeros(6, dtype=np.int32)
        raw = None
        if want_raw:    # (Hp, the pitch of a row pair, is the handle's and comes back in info: at most H + 15)
            raw = np.zeros((rows, self.N * (self.H + 15), 2), dtype=np.float32)
        self._chk(self.L.bioem_hip_debug_convolve_batch(self.h, _p(specP), nO, c0, nC, _p(conv), _p(params), _p(raw),
                                                        _p(info)), "debug_convolve_batch")
        info = dict(zip(("fused", "fast", "N1", "Hp", "rows", "guard"), map(int, info)))
        if raw is not None:
            raw = raw.reshape(-1)[:rows * self.N * info["Hp"] * 2].reshape(rows, self.N * info["Hp"], 2).copy()
        return conv, params, raw, info

    def debug_direct_conv(self, specConv, want_Z=True):
        """the c2r of a BIOEM_CC_DIRECT handle on conv spectra float32 [n, N, H, 2] in reference layout
        (bioem_hip_debug_direct_conv): (Z float64 [n, N, H, 2] of the column pass or None, the real maps float32 [n, N, N],
        unnormalised).  Invalid arguments raise with .rc == 2; the handle stays usable."""
        specConv = _spectra(specConv)
        assert specConv.ndim == 4 and specConv.shape[1:] == (self.N, self.H, 2), specConv.shape
        n = len(specConv)
        Z = np.zeros((n, self.N, self.H, 2), dtype=np.float64) if want_Z else None
        real = np.zeros((n, self.N, self.N), dtype=np.float32)
        self._chk(self.L.bioem_hip_debug_direct_conv(self.h, _p(specConv), n, _p(Z), _p(real)), "debug_direct_conv")
        return Z, real

    def debug_particles(self):
        spec = np.empty((self.nMaps, self.N, self.H, 2), dtype=np.float32)
        s = np.empty(self.nMaps, dtype=np.float32)
        s2 = np.empty(self.nMaps, dtype=np.float32)
        self._chk(self.L.bioem_hip_debug_particles(self.h, _p(spec), _p(s), _p(s2)), "debug_particles")
        return spec, s, s2

    def kernel_stats(self):
        ms, n, c = C.c_double(), C.c_longlong(), C.c_longlong()
        self._chk(self.L.bioem_hip_kernel_stats(self.h, C.byref(ms), C.byref(n), C.byref(c)), "kernel_stats")
        return ms.value, n.value, c.value

    def reset_kernel_stats(self):
        self._chk(self.L.bioem_hip_reset_kernel_stats(self.h), "reset_kernel_stats")


def r2c(images, device=0):
    """fftwf_plan_dft_r2c_2d of a stack of square float images on the device (bioem_hip_r2c): [n, N, N] -> complex64
    [n, N, N // 2 + 1], the kernels the projections and the particle maps go through."""
    L = load_library()
    images = np.ascontiguousarray(images, dtype=np.float32)
    n, N, _ = images.shape
    out = np.empty((n, N, N // 2 + 1), dtype=np.complex64)
    if L.bioem_hip_r2c(device, N, n, _p(images), _p(out)):
        raise RuntimeError("bioem_hip_r2c failed (N = %d, %d images)" % (N, n))
    return out


def merge_topk_host(cands, K=None):
    """Merge of per-shard candidate lists ([nMaps, W] each): the writer's heap rule over their union, [nMaps, K].
    K = None: K-wide lists (Engine.topk_angles), K = W; they reproduce the writer of the whole table only while no
    equal keys meet a shard's threshold.  With K given, the lists are Engine.merge_candidates' (W = 2K - 1, or any
    W >= K), which always reproduce it."""
    L = load_library()
    nMaps, W = cands[0].shape
    K = W if K is None else int(K)
    cands = [np.ascontiguousarray(c, dtype=CANDIDATE_DTYPE) for c in cands]
    assert all(c.shape == (nMaps, W) for c in cands)
    out = np.zeros((nMaps, K), dtype=CANDIDATE_DTYPE)
    arr = (C.c_void_p * len(cands))(*[c.ctypes.data for c in cands])
    if L.bioem_hip_merge_topk_host_wide(len(cands), nMaps, K, W, arr, _p(out)):
        raise RuntimeError("bioem_hip_merge_topk_host_wide failed")
    return out


def merge_rccl(engines, K=0, numconst=0.0):
    """bioem_hip_merge: RCCL all-gather + device fold of the engines' shards (one GPU per engine, this process).
    Returns (pmap [nMaps], candidates [nMaps, K] or None)."""
    L = load_library()
    nMaps = engines[0].nMaps
    pmap = np.zeros(nMaps, dtype=PROB_MAP_DTYPE)
    cand = np.zeros((nMaps, K), dtype=CANDIDATE_DTYPE) if K > 0 else None
    arr = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    rc = L.bioem_hip_merge(arr, len(engines), _p(pmap), K, float(numconst), _p(cand))
    if rc:
        raise RuntimeError("bioem_hip_merge: " + L.bioem_hip_last_error(engines[0].h).decode())
    return pmap, cand


def merge_host(blocks, nMaps, nAngles, writeAngles):
    """Host log-sum-exp merge of shard probability blocks (reference bioem.cpp:909-1044)."""
    L = load_library()
    out = np.zeros_like(blocks[0])
    arr = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
    rc = L.bioem_hip_merge_host(len(blocks), nMaps, nAngles, int(writeAngles), arr, _p(out))
    if rc:
        raise RuntimeError("bioem_hip_merge_host failed")
    return out


def merge_ctf_tables(tables):
    """Merge of the shards' CTF tables ([nCTF, nMaps] each, Engine.ctf_table; shards in ascending orientation-block
    order) by bioem_hip_merge_host, entry by entry: log-sum-exp of Total / Constoadd, the record of the lowest shard
    that holds the largest Constoadd."""
    L = load_library()
    tables = [np.ascontiguousarray(t, dtype=PROB_MAP_DTYPE) for t in tables]
    assert all(t.shape == tables[0].shape for t in tables)
    out = np.zeros_like(tables[0])
    arr = (C.c_void_p * len(tables))(*[t.ctypes.data for t in tables])
    if L.bioem_hip_merge_host(len(tables), tables[0].size, 0, 0, arr, _p(out)):
        raise RuntimeError("bioem_hip_merge_host failed")
    return out


def merge_orient_sums(sums):
    """Merge of the shards' orientation sums ([nMaps] of ORIENT_SUMS_DTYPE each, Engine.orientation_sums; shards in
    ascending orientation-block order) by bioem_hip_merge_orient_sums_host: the maximum m with ties to the lowest shard,
    every shard's sums rescaled by e^(m_s - m) and added in shard order.  No device."""
    L = load_library()
    sums = [np.ascontiguousarray(t, dtype=ORIENT_SUMS_DTYPE) for t in sums]
    assert sums and all(t.shape == sums[0].shape and t.ndim == 1 for t in sums)
    out = np.zeros_like(sums[0])
    arr = (C.c_void_p * len(sums))(*[t.ctypes.data for t in sums])
    if L.bioem_hip_merge_orient_sums_host(len(sums), sums[0].size, arr, _p(out) if out.size else None):
        raise RuntimeError("bioem_hip_merge_orient_sums_host failed")
    return out


def merge_orient_occupancy(blocks):
    """The shards' occupancy blocks (Engine.orientation_occupancy on every shard, with the merged sums handed in; shards
    in ascending orientation-block order) concatenated: rows are independent, so this is the unsharded result bit for
    bit.  No device."""
    blocks = [np.ascontiguousarray(b, dtype=ORIENT_OCC_DTYPE) for b in blocks]
    assert blocks and all(b.ndim == 1 for b in blocks)
    return np.concatenate(blocks)
