"""The density gradient of the log posterior per model point (Engine.model_gradient, the --ModelGradient text file).

Engine.model_gradient returns, per model point k, the sums over the requests r of a call (include/bioem_hip.h):
 sum = sum_r w_r g_rk,  sumsq = sum_r (w_r g_rk)^2,  sumw = sum_r w_r v_rk,  count = sum_r v_rk,
g_rk = d log P_r / d rho_k and v_rk = 1 where the projection of request r used the point.  derive() gives, in double,

 mean   sum / sumw, the weighted mean gradient over the requests that saw the point (0 where none did)
 z      sum / sqrt(sumsq): how consistently the requests pull the density one way; |z| <= sqrt(count)
 step   (with the footprint sums sigma_k) the steepest-ascent direction that keeps sum_k rho_k sigma_k, the
        normalisation of the projection, fixed: sum - sigma (sum . sigma) / (sigma . sigma)
 rho_dot_sum   sum_k rho_k sum_k: 0 analytically, because the normalisation removes the scale of rho
 norm   the Euclidean norm of sum

A posterior-weighted gradient needs no entry of its own.  For a particle take the top-K orientations of a run
(Engine.topk_angles), the window posterior of each (orientation, CTF set) pair (Engine.window_posterior) and
best_window.marginal over them: its normalised cell weights, multiplied by the pair's share of the particle's evidence,
are the weights w_r of the requests (particle, orientation, CTF set, cell shift) handed to Engine.model_gradient.

File layout: after the HEADER:: NOTATION bar, one notation line and the bar again, one line per model point
 POINT k x y z radius density sum mean z count
and one line
 DATASET rho_dot_sum norm nonfinite
nonfinite the number of requests whose coefficients a, b, g are not all finite; floating values with 17 significant
digits (a double survives the round trip)."""
import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"
NOTATION = "Notation: POINT k x y z radius density sum mean z count  |  DATASET rho_dot_sum norm nonfinite"

POINT_LINE_DTYPE = np.dtype([("pos", "<f8", (3,)), ("radius", "<f8"), ("density", "<f8"), ("sum", "<f8"), ("mean", "<f8"),
                             ("z", "<f8"), ("count", "<i8")])


def footprint_sums(points, pixel_size):
    """sigma_k of every model point: the sum of its footprint at unit density (bioem.cpp:1742-1790 with density 1; 1 for
    a point with radius <= pixel_size).  The float expressions of the reference in float32, the division and the sum in
    double, row by row."""
    f = np.float32
    px = f(pixel_size)
    out = np.ones(len(points), dtype=np.float64)
    for k, radius in enumerate(np.asarray(points["radius"], dtype=f)):
        if not radius > px:
            continue
        irad = int(radius / px) + 1
        d = np.arange(-irad, irad + 1)
        dist = ((d[:, None] * d[:, None]).astype(f) + (d[None, :] * d[None, :]).astype(f)) * px * px
        rad2 = radius * radius
        inside = dist < rad2
        with np.errstate(invalid="ignore"):
            num = ((px * px) * f(2)) * np.sqrt(np.where(inside, rad2 - dist, f(0)).astype(f)) * f(3)
        w = num.astype(np.float64) / (((4 * np.pi) * float(radius)) * float(rad2))
        s = 0.0
        for x in w[inside].tolist():
            s += x
        out[k] = s
    return out


def derive(acc, points, sigma=None, pixel_size=None):
    """the statistics above from acc (GRAD_POINT_DTYPE [nPts]) and the model's points; step needs sigma (float64 [nPts])
    or pixel_size (then footprint_sums), else it is None"""
    total = np.asarray(acc["sum"], dtype=np.float64)
    sumsq, sumw = np.asarray(acc["sumsq"], dtype=np.float64), np.asarray(acc["sumw"], dtype=np.float64)
    with np.errstate(all="ignore"):
        mean = np.where(sumw != 0, total / np.where(sumw != 0, sumw, 1.0), 0.0)
        z = np.where(sumsq > 0, total / np.sqrt(np.where(sumsq > 0, sumsq, 1.0)), 0.0)
    if sigma is None and pixel_size is not None:
        sigma = footprint_sums(points, pixel_size)
    step = None
    if sigma is not None:
        sigma = np.asarray(sigma, dtype=np.float64)
        step = total - sigma * (float(np.dot(total, sigma)) / float(np.dot(sigma, sigma)))
    rho = np.asarray(points["density"], dtype=np.float64)
    return {"mean": mean, "z": z, "step": step, "rho_dot_sum": float(np.dot(rho, total)),
            "norm": float(np.sqrt((total ** 2).sum()))}


def nonfinite_requests(coef):
    """requests whose coefficients (a, b, g) of Engine.model_gradient's "coef" are not all finite"""
    return int(np.count_nonzero(~np.isfinite(np.asarray(coef, dtype=np.float64)[:, :3]).all(axis=1)))


def write(path, points, acc, nonfinite=0):
    d = derive(acc, points)
    with open(path, "w") as f:
        f.write("%s\n%s\n%s\n" % (BAR, NOTATION, BAR))
        for k in range(len(points)):
            p = points[k]
            f.write("POINT %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n" % (
                k, p["pos"][0], p["pos"][1], p["pos"][2], p["radius"], p["density"], acc["sum"][k], d["mean"][k], d["z"][k],
                int(acc["count"][k])))
        f.write("DATASET %.17g %.17g %d\n" % (d["rho_dot_sum"], d["norm"], int(nonfinite)))


def parse(path):
    """{"points": POINT_LINE_DTYPE [nPts], "dataset": {"rho_dot_sum", "norm", "nonfinite"}}; ValueError on a file that is
    not of the layout above"""
    rows, dataset = [], None
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0] not in ("POINT", "DATASET"):
                continue
            if t[0] == "POINT":
                if len(t) != 11 or int(t[1]) != len(rows):
                    raise ValueError("%s: bad POINT line: %r" % (path, line))
                v = [float(x) for x in t[2:10]]
                rows.append((v[0:3], v[3], v[4], v[5], v[6], v[7], int(t[10])))
            else:
                if len(t) != 4 or dataset is not None:
                    raise ValueError("%s: bad DATASET line: %r" % (path, line))
                dataset = {"rho_dot_sum": float(t[1]), "norm": float(t[2]), "nonfinite": int(t[3])}
    if dataset is None:
        raise ValueError("%s: no DATASET line" % path)
    return {"points": np.array(rows, dtype=POINT_LINE_DTYPE), "dataset": dataset}
