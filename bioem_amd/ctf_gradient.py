"""The CTF gradient and curvature of the log posterior per match (Engine.ctf_gradient, the --CTFGradient file;
include/bioem_hip.h).  numpy only, no device.

Engine.ctf_gradient returns per request a row of CTF_GRAD_DTYPE: theta = (amp, pha, env) of the request's CTF set, gData [3]
and HData [6] (upper triangle aa, ap, ae, pp, pe, ee), the derivatives of the data's part of log P, and gPrior [3], HPrior [3]
(a diagonal) those of the reference's -prior, whose signs are unusual: every function here leaves the prior out unless asked.

 gradient, hessian   g [3] and the symmetric H [3, 3] of a row
 newton_step         the Newton step -H^-1 g on the chosen axes; None where the restricted Hessian is not negative definite
 sigma               the Laplace error bar: sqrt(-1 / H) on one axis, sqrt(diag((-H)^-1)) on several; None as above
 to_defocus          pha = defocus[micro-m] 2 pi 1e4 lambda (the host's conversion): defocus, gradient and curvature per
                     micro-m, the Newton defocus and its sigma
 group_sums          gradient and Hessian summed per group (micrograph) in request order, plain float64
 derive, lines       the columns of the text file

Text layout: after the HEADER:: NOTATION bar, one notation line and the bar again, one line per particle
 CTFGRAD particle orient conv shiftX shiftY amp defocus env g_amp g_defocus g_env H_aa H_ad H_ae H_dd H_de H_ee
         newton_defocus sigma_defocus
(the CTF columns as --ProbCTF prints them, defocus in micro-m; gradient and Hessian of the data's part in those units; the
Newton defocus along the defocus axis alone and its sigma, nan where the curvature H_dd is not negative) and one line
 DATASET particles defined rms_g_defocus
floating values with 17 significant digits (a double survives the round trip)."""
import numpy as np

AXES = ("amp", "pha", "env")
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
BAR = "************************* HEADER:: NOTATION *******************************************"
NOTATION = ("Notation: CTFGRAD particle orient conv shiftX shiftY CTFamp CTFdefocus[micro-m] CTFB-Env g_amp g_defocus g_env "
            "H_aa H_ad H_ae H_dd H_de H_ee newton_defocus sigma_defocus  |  DATASET particles defined rms_g_defocus")

CTF_LINE_DTYPE = np.dtype([("particle", "<i8"), ("orient", "<i8"), ("conv", "<i8"), ("shiftX", "<i8"), ("shiftY", "<i8"),
                           ("ctf", "<f8", (3,)), ("g", "<f8", (3,)), ("H", "<f8", (6,)), ("newton", "<f8"), ("sigma", "<f8")])


def _axes(axes):
    idx = [AXES.index(a) for a in axes]
    if not idx or len(set(idx)) != len(idx):
        raise ValueError("axes: one or more of %s, each once" % (AXES,))
    return idx


def gradient(row, with_prior=False):
    """g float64 [3] of a row"""
    g = np.array(row["gData"], dtype=np.float64)
    return g + np.asarray(row["gPrior"], dtype=np.float64) if with_prior else g


def hessian(row, with_prior=False):
    """the symmetric H float64 [3, 3] of a row"""
    H = np.zeros((3, 3))
    for p, (a, b) in enumerate(PAIRS):
        H[a, b] = H[b, a] = float(row["HData"][p])
    if with_prior:
        for a in range(3):
            H[a, a] = H[a, a] + float(row["HPrior"][a])
    return H


def _restricted(g, H, axes):
    idx = _axes(axes)
    g, H = np.asarray(g, dtype=np.float64)[idx], np.asarray(H, dtype=np.float64)[np.ix_(idx, idx)]
    if not (np.isfinite(g).all() and np.isfinite(H).all()) or not (np.linalg.eigvalsh(H) < 0.0).all():
        return g, None
    return g, H


def newton_step(row, axes=("pha",), with_prior=False):
    """the Newton step float64 [len(axes)] towards the maximum of the quadratic model on the chosen axes; None where the
    restricted Hessian is not negative definite (no maximum) or a value is not finite"""
    g, H = _restricted(gradient(row, with_prior), hessian(row, with_prior), axes)
    if H is None:
        return None
    return -g / H[0, 0] if len(g) == 1 else -np.linalg.solve(H, g)


def sigma(row, axes=("pha",), with_prior=False):
    """the Laplace error bar float64 [len(axes)]: sqrt(-1 / H) on one axis, sqrt(diag((-H)^-1)) on several; None as for
    newton_step"""
    g, H = _restricted(gradient(row, with_prior), hessian(row, with_prior), axes)
    if H is None:
        return None
    return np.sqrt(-1.0 / H[0]) if len(g) == 1 else np.sqrt(np.diag(np.linalg.inv(-H)))


def chain_factor(wavelength):
    """d pha / d defocus[micro-m] = 2 pi 1e4 lambda, lambda the float electron wavelength in Angstrom (the host's expression)"""
    return np.pi * 2.0 * 10000 * float(np.float32(wavelength))


def to_defocus(row, wavelength, with_prior=False):
    """the defocus axis of a row in micro-m: {"defocus", "g" = d log P / d defocus, "H" = its curvature, "newton" the Newton
    defocus, "sigma" its Laplace error bar}; the last two nan where the curvature is not negative"""
    c = chain_factor(wavelength)
    g, H = gradient(row, with_prior)[1] * c, hessian(row, with_prior)[1, 1] * c * c
    defocus = float(row["theta"][1]) / c
    ok = np.isfinite(g) and np.isfinite(H) and H < 0.0
    return {"defocus": defocus, "g": g, "H": H, "newton": defocus - g / H if ok else float("nan"),
            "sigma": float(np.sqrt(-1.0 / H)) if ok else float("nan")}


def group_sums(rows, group_of, weights=None, with_prior=False):
    """gradient and Hessian summed over the rows of each group (a micrograph's particles): {"groups" the sorted group
    labels [k], "g" float64 [k, 3], "H" float64 [k, 3, 3], "count" int64 [k]}, row after row in request order in plain
    float64, each row times its weight (None: 1)"""
    rows = np.asarray(rows)
    group_of = np.asarray(group_of).reshape(-1)
    if len(group_of) != len(rows):
        raise ValueError("group_of: one label per row")
    w = np.ones(len(rows)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(rows):
        raise ValueError("weights: one per row")
    groups = np.unique(group_of)
    at = {g: i for i, g in enumerate(groups.tolist())}
    G, H, count = np.zeros((len(groups), 3)), np.zeros((len(groups), 3, 3)), np.zeros(len(groups), dtype=np.int64)
    for r, lab, wr in zip(rows, group_of.tolist(), w.tolist()):
        i = at[lab]
        G[i] = G[i] + wr * gradient(r, with_prior)
        H[i] = H[i] + wr * hessian(r, with_prior)
        count[i] += 1
    return {"groups": groups, "g": G, "H": H, "count": count}


def derive(rows, wavelength):
    """the columns of the text file from the rows of Engine.ctf_gradient (CTF_GRAD_DTYPE [n]), data part only: "ctf" [n, 3]
    (amp, defocus, env), "g" [n, 3], "H" [n, 6] in the printed units, "newton", "sigma" [n] (nan where undefined), and over
    the data set "defined", "rms_g_defocus" """
    rows = np.asarray(rows)
    n = len(rows)
    c = chain_factor(wavelength)
    unit = np.array([1.0, c, 1.0])   # d theta / d printed
    ctf = np.asarray(rows["theta"], dtype=np.float64).reshape(n, 3) / unit
    g = np.asarray(rows["gData"], dtype=np.float64).reshape(n, 3) * unit
    H = np.asarray(rows["HData"], dtype=np.float64).reshape(n, 6) * np.array([unit[a] * unit[b] for a, b in PAIRS])
    newton, sig = np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        if np.isfinite(g[i, 1]) and np.isfinite(H[i, 3]) and H[i, 3] < 0.0:
            newton[i] = ctf[i, 1] - g[i, 1] / H[i, 3]
            sig[i] = np.sqrt(-1.0 / H[i, 3])
    return {"ctf": ctf, "g": g, "H": H, "newton": newton, "sigma": sig, "defined": int(np.isfinite(newton).sum()),
            "rms_g_defocus": float(np.sqrt(sum((g[:, 1] * g[:, 1]).tolist()) / max(1, n)))}


def lines(rows, requests, wavelength):
    """CTF_LINE_DTYPE [n] of the rows of Engine.ctf_gradient and their requests (GRAD_REQUEST_DTYPE [n])"""
    d = derive(rows, wavelength)
    out = np.zeros(len(rows), dtype=CTF_LINE_DTYPE)
    for f in ("particle", "orient", "conv", "shiftX", "shiftY"):
        out[f] = requests[f]
    out["ctf"], out["g"], out["H"], out["newton"], out["sigma"] = d["ctf"], d["g"], d["H"], d["newton"], d["sigma"]
    return out


def write(path, table):
    """the text file of CTF_LINE_DTYPE [n] (lines())"""
    table = np.asarray(table, dtype=CTF_LINE_DTYPE)
    n = max(1, len(table))
    gd = table["g"][:, 1] if len(table) else np.zeros(0)
    with open(path, "w") as f:
        f.write("%s\n%s\n%s\n" % (BAR, NOTATION, BAR))
        for r in table:
            f.write(("CTFGRAD %d %d %d %d %d" + " %.17g" * 14 + "\n") % (
                (r["particle"], r["orient"], r["conv"], r["shiftX"], r["shiftY"]) + tuple(r["ctf"]) + tuple(r["g"]) +
                tuple(r["H"]) + (r["newton"], r["sigma"])))
        f.write("DATASET %d %d %.17g\n" % (len(table), int(np.isfinite(table["newton"]).sum()),
                                          np.sqrt(sum((gd * gd).tolist()) / n)))


def parse(path):
    """{"ctfgrad": CTF_LINE_DTYPE [n], "dataset": {"particles", "defined", "rms_g_defocus"}}; ValueError on a file that is not
    of the layout above"""
    rows, dataset = [], None
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0] not in ("CTFGRAD", "DATASET"):
                continue
            if t[0] == "CTFGRAD":
                if len(t) != 20:
                    raise ValueError("%s: bad CTFGRAD line: %r" % (path, line))
                v = [float(x) for x in t[6:20]]
                rows.append(tuple(int(x) for x in t[1:6]) + (tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:12]), v[12], v[13]))
            else:
                if len(t) != 4 or dataset is not None:
                    raise ValueError("%s: bad DATASET line: %r" % (path, line))
                dataset = {"particles": int(t[1]), "defined": int(t[2]), "rms_g_defocus": float(t[3])}
    if dataset is None:
        raise ValueError("%s: no DATASET line" % path)
    if dataset["particles"] != len(rows):
        raise ValueError("%s: DATASET counts %d particles, %d CTFGRAD lines" % (path, dataset["particles"], len(rows)))
    return {"ctfgrad": np.array(rows, dtype=CTF_LINE_DTYPE), "dataset": dataset}
