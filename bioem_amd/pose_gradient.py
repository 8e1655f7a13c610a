"""The pose gradient of the log posterior for a volume model (Engine.pose_gradient, the --PoseGradient file;
include/bioem_hip.h).  numpy only, no device.

Engine.pose_gradient returns per request J [2, 3] = d log P / d R[i][j] for rows 0 and 1 of the orientation matrix R (row 2
does not enter the slice), T [2] = d log P / d (shiftX, shiftY), <C, A_r> and R itself.  With the small rotation R' = (I +
G(w)) R in the frame of the image, G(w) = [[0, -w2, w1], [w2, 0, -w0], [-w1, w0, 0]] (w2 the in-plane angle, w0 and w1 the
tilts), the chain rule gives

 rotation_gradient   g_w = (-J[1].R[2], J[0].R[2], J[1].R[0] - J[0].R[1]), every dot product as (x0 y0 + x1 y1) + x2 y2
 small_rotation      the stored quaternion d (x, y, z, w) with M(d) = exp(G(w)), M the matrix the engine builds from a stored
                     quaternion: d = (-sin(|w| / 2) w / |w|, cos(|w| / 2))
 step                refine.compose of q with small_rotation(w): M(step(q, w)) = exp(G(w)) M(q), rounded to float
 line_lists          per particle its seed and the seed stepped along g_w / |g_w|: an ascent line for the own-list pass
 derive              |g_w| per degree, its unit axis, |T| per request, and their root mean squares over the data set

Text layout: after the HEADER:: NOTATION bar, one notation line and the bar again, one line per request
 POSE particle orient q0 q1 q2 q3 conv shiftX shiftY gw0 gw1 gw2 gdeg T0 T1 dot
(q the four numbers of the orientation widened to double, gdeg = |g_w| pi / 180: the change of log P per degree along the
ascent axis) and one line
 DATASET particles rms_gdeg rms_T
floating values with 17 significant digits (a double survives the round trip)."""
import numpy as np

from . import refine

BAR = "************************* HEADER:: NOTATION *******************************************"
NOTATION = ("Notation: POSE particle orient q0 q1 q2 q3 conv shiftX shiftY gw0 gw1 gw2 gdeg T0 T1 dot  |  "
            "DATASET particles rms_gdeg rms_T")
RAD_PER_DEG = np.pi / 180.0

POSE_LINE_DTYPE = np.dtype([("particle", "<i8"), ("orient", "<i8"), ("q", "<f8", (4,)), ("conv", "<i8"), ("shiftX", "<i8"),
                            ("shiftY", "<i8"), ("g", "<f8", (3,)), ("gdeg", "<f8"), ("T", "<f8", (2,)), ("dot", "<f8")])


def generator(omega):
    """G(w) float64 [..., 3, 3]"""
    w = np.asarray(omega, dtype=np.float64)
    G = np.zeros(w.shape[:-1] + (3, 3))
    G[..., 0, 1], G[..., 0, 2] = -w[..., 2], w[..., 1]
    G[..., 1, 0], G[..., 1, 2] = w[..., 2], -w[..., 0]
    G[..., 2, 0], G[..., 2, 1] = -w[..., 1], w[..., 0]
    return G


def _dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def rotation_gradient(J, R):
    """g_w float64 [..., 3] from J [..., 2, 3] and R [..., 3, 3]"""
    J, R = np.asarray(J, dtype=np.float64), np.asarray(R, dtype=np.float64)
    return np.stack([-_dot3(J[..., 1, :], R[..., 2, :]), _dot3(J[..., 0, :], R[..., 2, :]),
                     _dot3(J[..., 1, :], R[..., 0, :]) - _dot3(J[..., 0, :], R[..., 1, :])], axis=-1)


def small_rotation(omega):
    """the stored quaternion (x, y, z, w) float64 [4] of exp(G(omega)); omega = 0 gives (0, 0, 0, 1) exactly"""
    w = np.asarray(omega, dtype=np.float64).reshape(3)
    angle = float(np.sqrt((w * w).sum()))
    if angle == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    s = -np.sin(0.5 * angle) / angle
    return np.array([s * w[0], s * w[1], s * w[2], np.cos(0.5 * angle)])


def step(q, omega):
    """the stored quaternion q (x, y, z, w) turned by omega in the frame of the image, float32 [4]; omega = 0 gives q bit for
    bit"""
    q = np.asarray(q).reshape(1, 4)
    return refine.compose(q, small_rotation(omega)[None])[0, 0]


def line_lists(angles, pmap, g_omega, steps_rad, isQuat=True):
    """(flat float32 [n, 4], offsets int64 [nMaps + 1]) for Engine.upload_particle_orientation_lists: per particle p its seed
    angles[pmap["orient"][p]] first, bit for bit, then the seed stepped by s g / |g| for every s of steps_rad, g =
    g_omega[p]; the seed alone where |g| is zero or not finite.  Euler lists (isQuat false, or three columns) raise
    ValueError: the steps are composed as quaternions."""
    angles = np.asarray(angles)
    if not isQuat or angles.ndim != 2 or angles.shape[1] != 4:
        raise ValueError("line_lists needs a quaternion list [n, 4]: Euler angles are not composed")
    seeds = np.asarray(angles[np.asarray(pmap["orient"], dtype=np.int64)], dtype=np.float32)
    g = np.asarray(g_omega, dtype=np.float64).reshape(len(seeds), 3)
    steps = np.asarray(steps_rad, dtype=np.float64).reshape(-1)
    parts, offsets = [], [0]
    for q, gp in zip(seeds, g):
        rows = [q]
        norm = float(np.sqrt((gp * gp).sum()))
        if np.isfinite(norm) and norm > 0.0:
            rows += [step(q, s * (gp / norm)) for s in steps]
        parts.append(np.array(rows, dtype=np.float32))
        offsets.append(offsets[-1] + len(rows))
    flat = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), dtype=np.float32)
    return np.ascontiguousarray(flat, dtype=np.float32), np.asarray(offsets, dtype=np.int64)


def derive(rows):
    """from the rows of Engine.pose_gradient (POSE_GRAD_DTYPE [n]): "g" [n, 3] = g_w, "gdeg" [n] = |g_w| per degree, "axis"
    [n, 3] its unit axis (0 where |g_w| is 0), "tnorm" [n] = |T|, and over the data set "rms_gdeg", "rms_T" """
    rows = np.asarray(rows)
    g = rotation_gradient(rows["J"], rows["R"])
    norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    with np.errstate(all="ignore"):
        axis = np.where(norm[:, None] > 0.0, g / np.where(norm > 0.0, norm, 1.0)[:, None], 0.0)
    T = np.asarray(rows["T"], dtype=np.float64)
    tnorm = np.sqrt(T[:, 0] * T[:, 0] + T[:, 1] * T[:, 1])
    gdeg = norm * RAD_PER_DEG
    n = max(1, len(rows))
    return {"g": g, "gdeg": gdeg, "axis": axis, "tnorm": tnorm,
            "rms_gdeg": float(np.sqrt(sum((gdeg * gdeg).tolist()) / n)), "rms_T": float(np.sqrt(sum((tnorm * tnorm).tolist()) / n))}


def lines(rows, requests, angles):
    """POSE_LINE_DTYPE [n] of the rows of Engine.pose_gradient, their requests (GRAD_REQUEST_DTYPE [n]) and the four numbers
    of each request's orientation, float32 [n, 4]"""
    d = derive(rows)
    out = np.zeros(len(rows), dtype=POSE_LINE_DTYPE)
    for f in ("particle", "orient", "conv", "shiftX", "shiftY"):
        out[f] = requests[f]
    out["q"] = np.asarray(angles, dtype=np.float32).reshape(len(rows), 4).astype(np.float64)
    out["g"], out["gdeg"], out["T"], out["dot"] = d["g"], d["gdeg"], rows["T"], rows["dot"]
    return out


def write(path, table):
    """the text file of POSE_LINE_DTYPE [n] (lines())"""
    table = np.asarray(table, dtype=POSE_LINE_DTYPE)
    tn2 = table["T"][:, 0] * table["T"][:, 0] + table["T"][:, 1] * table["T"][:, 1]
    n = max(1, len(table))
    with open(path, "w") as f:
        f.write("%s\n%s\n%s\n" % (BAR, NOTATION, BAR))
        for r in table:
            f.write("POSE %d %d %.17g %.17g %.17g %.17g %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (
                (r["particle"], r["orient"]) + tuple(r["q"]) + (r["conv"], r["shiftX"], r["shiftY"]) + tuple(r["g"]) +
                (r["gdeg"],) + tuple(r["T"]) + (r["dot"],)))
        f.write("DATASET %d %.17g %.17g\n" % (len(table), np.sqrt(sum((table["gdeg"] * table["gdeg"]).tolist()) / n),
                                            np.sqrt(sum(tn2.tolist()) / n)))


def parse(path):
    """{"pose": POSE_LINE_DTYPE [n], "dataset": {"particles", "rms_gdeg", "rms_T"}}; ValueError on a file that is not of the
    layout above"""
    rows, dataset = [], None
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0] not in ("POSE", "DATASET"):
                continue
            if t[0] == "POSE":
                if len(t) != 17:
                    raise ValueError("%s: bad POSE line: %r" % (path, line))
                v = [float(x) for x in t[3:7]] + [float(x) for x in t[10:17]]
                rows.append((int(t[1]), int(t[2]), tuple(v[:4]), int(t[7]), int(t[8]), int(t[9]), tuple(v[4:7]), v[7],
                             tuple(v[8:10]), v[10]))
            else:
                if len(t) != 4 or dataset is not None:
                    raise ValueError("%s: bad DATASET line: %r" % (path, line))
                dataset = {"particles": int(t[1]), "rms_gdeg": float(t[2]), "rms_T": float(t[3])}
    if dataset is None:
        raise ValueError("%s: no DATASET line" % path)
    if dataset["particles"] != len(rows):
        raise ValueError("%s: DATASET counts %d particles, %d POSE lines" % (path, dataset["particles"], len(rows)))
    return {"pose": np.array(rows, dtype=POSE_LINE_DTYPE), "dataset": dataset}
