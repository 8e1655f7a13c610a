"""The --ProbCTF text file: the posterior per particle and CTF set (the CTF table of bioem_hip_enable_ctf_table, merged
over shards, as the CLI writes it).

After the HEADER:: NOTATION bar, one notation line and the bar again, one line per (particle, CTF set), particle-major,
fixed with 4 decimals:

 i c k0 k1' k2 logP Separated: log(Total) Constoadd numconst Best: A cx cy norm mu

k0 k1' k2 are the CTF set as the "Maximizing Param" line of Output_Probabilities prints it (defocus in micro-m, PSF
parameters as they are), logP = log(Total) + Constoadd + numconst with the constant of the particle's LogProb, and A the
orientation of the best match under that CTF set: 4 numbers with quaternions, 3 otherwise."""
import numpy as np

BAR = "************************* HEADER:: NOTATION *******************************************"


def row_dtype(nA):
    return np.dtype([("particle", "<i4"), ("ctf", "<i4"), ("k", "<f8", (3,)), ("logP", "<f8"), ("logTotal", "<f8"),
                     ("Constoadd", "<f8"), ("numconst", "<f8"), ("A", "<f8", (nA,)), ("cent_x", "<i4"), ("cent_y", "<i4"),
                     ("norm", "<f8"), ("mu", "<f8")])


def parse(path):
    """Returns (rows [nMaps, nCTF] of row_dtype(4 or 3), notation line).  Raises ValueError for a file that is not of the
    layout above: a missing header, a malformed line, lines that are not particle-major over a full rectangle."""
    with open(path) as f:
        lines = f.read().split("\n")
    if len(lines) < 3 or lines[0] != BAR or lines[2] != BAR:
        raise ValueError("%s: no HEADER:: NOTATION bar around the notation line" % path)
    notation = lines[1]
    recs, nA = [], None
    for ln in lines[3:]:
        if not ln.strip():
            continue
        t = ln.split()
        if len(t) not in (18, 19) or t[6] != "Separated:" or t[10] != "Best:":
            raise ValueError("%s: malformed line %r" % (path, ln))
        n = len(t) - 15
        if nA is None:
            nA = n
        elif n != nA:
            raise ValueError("%s: lines with 3 and with 4 orientation numbers" % path)
        recs.append((int(t[0]), int(t[1]), tuple(float(x) for x in t[2:5]), float(t[5]), float(t[7]), float(t[8]),
                     float(t[9]), tuple(float(x) for x in t[11:11 + n]), int(t[11 + n]), int(t[12 + n]),
                     float(t[13 + n]), float(t[14 + n])))
    if not recs:
        raise ValueError("%s: no entries" % path)
    rows = np.array(recs, dtype=row_dtype(nA))
    nCTF = int(rows["ctf"].max()) + 1
    if len(rows) % nCTF:
        raise ValueError("%s: %d lines are no multiple of %d CTF sets" % (path, len(rows), nCTF))
    rows = rows.reshape(-1, nCTF)
    if (rows["particle"] != np.arange(rows.shape[0])[:, None]).any() or (rows["ctf"] != np.arange(nCTF)[None, :]).any():
        raise ValueError("%s: lines are not particle-major over all (particle, CTF set) pairs" % path)
    return rows, notation


def numconst(Ntotpi, volu):
    """the constant of a LogProb line: 0.5 log(pi) + (1 - Ntotpi / 2)(log(2 pi) + 1) + log(volu), volu as the float the
    device parameters hold"""
    return (0.5 * np.log(np.pi) + (1.0 - float(np.float32(Ntotpi)) * 0.5) * (np.log(2.0 * np.pi) + 1.0)
            + np.log(np.asarray(volu, dtype=np.float32).astype(np.float64)))


def ctf_columns(ctfParam, usepsf=False, elecwavel=0.019688):
    """[nCTF, 3] as the file prints them: CTF mode converts the phase to a defocus in micro-m"""
    k = np.asarray(ctfParam, dtype=np.float32).astype(np.float64).copy()
    if not usepsf:
        k[:, 1] = np.asarray(ctfParam, dtype=np.float32)[:, 1] / np.float32(2.0)
        k[:, 1] = k[:, 1] / np.pi / float(np.float32(elecwavel)) * 0.0001
    return k


def rows_from_table(table, ctfParam, angles, Ntotpi, volu, usepsf=False, elecwavel=0.019688, isQuat=True,
                    angles_per_map=0):
    """what the writer prints for a CTF table [nCTF, nMaps] (PROB_MAP_DTYPE), before rounding to 4 decimals: rows
    [nMaps, nCTF] of row_dtype.  volu: one value or one per map."""
    table = np.asarray(table)
    nCTF, nMaps = table.shape
    nA = 4 if isQuat else 3
    ang = np.asarray(angles, dtype=np.float32).reshape(-1, 4)
    rows = np.zeros((nMaps, nCTF), dtype=row_dtype(nA))
    nc = np.broadcast_to(numconst(Ntotpi, volu), (nMaps,))
    k = ctf_columns(ctfParam, usepsf, elecwavel)
    t = table.T
    rows["particle"] = np.arange(nMaps)[:, None]
    rows["ctf"] = np.arange(nCTF)[None, :]
    rows["k"] = k[None, :, :]
    with np.errstate(divide="ignore"):
        rows["logTotal"] = np.log(t["Total"])
    rows["Constoadd"] = t["Constoadd"]
    rows["numconst"] = nc[:, None]
    rows["logP"] = rows["logTotal"] + rows["Constoadd"] + rows["numconst"]
    rows["A"] = ang[t["orient"] + angles_per_map * np.arange(nMaps)[:, None]][..., :nA]
    for a, b in (("cent_x", "cent_x"), ("cent_y", "cent_y"), ("norm", "norm"), ("mu", "mu")):
        rows[a] = t[b]
    return rows


def particle_logp(rows):
    """per particle, the log-sum-exp of the logP column over the CTF sets: its LogProb"""
    lp = rows["logP"]
    m = lp.max(axis=1)
    return m + np.log(np.exp(lp - m[:, None]).sum(axis=1))
