"""The density gradient of the log posterior per voxel of a volume model (Engine.volume_gradient, the --VolumeGradient
files; include/bioem_hip.h).

Engine.volume_gradient returns g [N, N, N] = sum_r w_r d log P_r / d vol[x], the derivative with respect to the array handed
to Engine.upload_model_volume at a fixed centre.  derive() gives, in double,

 vol_dot_g   sum_x vol[x] g[x]: scaling the density scales the projection, so analytically it is -sum_r w_r
 norm        the Euclidean norm of g
 shells      per shell s (the voxels whose distance from the origin voxel (N + 1) // 2 rounds to s): voxels, sum of g,
             power = sum of g^2, vol_dot_g = sum of vol g
 step        the steepest-ascent direction that keeps the total density sum_x vol[x] fixed: g - mean(g)

The gradient volume is written with reconstruct.write_mrc, so it overlays the model file voxel for voxel.  Text layout:
after the HEADER:: NOTATION bar, one notation line and the bar again, one line per shell that holds voxels
 SHELL s voxels sum power vol_dot_g
and one line
 DATASET vol_dot_g norm requests sumw nonfinite
nonfinite the number of requests whose coefficients a, b, g are not all finite; floating values with 17 significant
digits (a double survives the round trip)."""
import numpy as np

from . import reconstruct

BAR = "************************* HEADER:: NOTATION *******************************************"
NOTATION = "Notation: SHELL s voxels sum power vol_dot_g  |  DATASET vol_dot_g norm requests sumw nonfinite"

SHELL_LINE_DTYPE = np.dtype([("s", "<i8"), ("voxels", "<i8"), ("sum", "<f8"), ("power", "<f8"), ("vol_dot_g", "<f8")])


def shell_index(N):
    """the shell of every voxel, int64 [N, N, N]"""
    x = np.arange(N) - (int(N) + 1) // 2
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    return np.floor(np.sqrt(r2.astype(np.float64)) + 0.5).astype(np.int64)


def derive(g, vol):
    """the statistics above from the gradient g and the model's volume, both [N, N, N]"""
    g = np.asarray(g, dtype=np.float64)
    vol = np.asarray(vol, dtype=np.float32).astype(np.float64)
    N = g.shape[0]
    assert g.shape == (N, N, N) and vol.shape == g.shape
    s = shell_index(N).ravel()
    n = int(s.max()) + 1
    fold = lambda x: np.bincount(s, weights=x.ravel(), minlength=n)
    voxels = np.bincount(s, minlength=n)
    keep = voxels > 0
    shells = np.zeros(int(keep.sum()), dtype=SHELL_LINE_DTYPE)
    shells["s"], shells["voxels"] = np.nonzero(keep)[0], voxels[keep]
    shells["sum"], shells["power"], shells["vol_dot_g"] = fold(g)[keep], fold(g * g)[keep], fold(vol * g)[keep]
    return {"vol_dot_g": float((vol * g).sum()), "norm": float(np.sqrt((g * g).sum())), "shells": shells,
            "step": g - g.mean()}


def write(path, g, vol, pixel_size=1.0, requests=0, sumw=0.0, nonfinite=0):
    """path + ".mrc" (the gradient, rounded to float) and the text file path"""
    d = derive(g, vol)
    reconstruct.write_mrc(path + ".mrc", np.asarray(g, dtype=np.float64).astype(np.float32), pixel_size)
    with open(path, "w") as f:
        f.write("%s\n%s\n%s\n" % (BAR, NOTATION, BAR))
        for r in d["shells"]:
            f.write("SHELL %d %d %.17g %.17g %.17g\n" % (r["s"], r["voxels"], r["sum"], r["power"], r["vol_dot_g"]))
        f.write("DATASET %.17g %.17g %d %.17g %d\n" % (d["vol_dot_g"], d["norm"], int(requests), float(sumw), int(nonfinite)))


def parse(path):
    """{"shells": SHELL_LINE_DTYPE [n], "dataset": {"vol_dot_g", "norm", "requests", "sumw", "nonfinite"}}; ValueError on a
    file that is not of the layout above"""
    rows, dataset = [], None
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0] not in ("SHELL", "DATASET"):
                continue
            if t[0] == "SHELL":
                if len(t) != 6 or (rows and int(t[1]) <= rows[-1][0]):
                    raise ValueError("%s: bad SHELL line: %r" % (path, line))
                rows.append((int(t[1]), int(t[2]), float(t[3]), float(t[4]), float(t[5])))
            else:
                if len(t) != 6 or dataset is not None:
                    raise ValueError("%s: bad DATASET line: %r" % (path, line))
                dataset = {"vol_dot_g": float(t[1]), "norm": float(t[2]), "requests": int(t[3]), "sumw": float(t[4]),
                           "nonfinite": int(t[5])}
    if dataset is None:
        raise ValueError("%s: no DATASET line" % path)
    return {"shells": np.array(rows, dtype=SHELL_LINE_DTYPE), "dataset": dataset}
