"""Posterior-weighted view sums (Engine.view_sums_soft, Engine.reconstruct_soft; include/bioem_hip.h): what
the host does around the device's accumulation -- which (particle, orientation, CTF set) requests carry a particle's
posterior mass, the weight of every window cell of every request, the least-squares norm and mu of every cell, and from
these the members and tables the device reads.

For the cell (X_i, X_j) of request r = (p, o, c) with the log posterior logp_r[i][j] of window_posterior:

    w_r[i][j] = exp(logp_r[i][j] + log_prior[o] - logZ_p)      logZ_p: the log-sum-exp over all cells of all requests of p
    norm, mu  = the least-squares values of the cell (cell_params): the expression the fold applies to the arg-max cell
    a = W_p w norm      s2 = W_p sum w norm^2      b = W_p sum w norm mu      mass = W_p sum w       (W_p = weights[p])

so the masses of a particle's members add up to W_p.  A cell whose logp, norm or mu is not finite gets weight 0; a
particle without a finite cell is left out (group -1, an all-zero table).  This is a profile-likelihood convention: every
cell enters with its own arg-max norm and mu, where the posterior the run integrates has them marginalised.

The text the CLI's --ReconstructSoft adds to the --Reconstruct file, after that file's DATASET line: per particle one line

 SOFT p requests n_eff mass_argmax

(requests: the (orientation, CTF set) pairs of particle p; n_eff = 1 / sum w^2 over (orientation, CTF set, cell);
mass_argmax: the largest w) and per shell of the two soft half maps one line

 SOFTSHELL s resolution weight FSC cross powA powB

in the columns of the file's SHELL lines, floating values with 16 significant digits."""
import numpy as np

from . import reconstruct as _rc
from .engine import MIN_PROB, PARAM5_DTYPE, SOFT_MEMBER_DTYPE, WINDOW_REQUEST_DTYPE

PARTICLE_DTYPE = np.dtype([("particle", "<i4"), ("requests", "<i4"), ("n_eff", "<f8"), ("mass_argmax", "<f8")])


def cell_params(cc, params, sum_ref, N):
    """(norm, mu) float64 of cc's shape [n, nd, nd]: the least-squares normalisation and offset at every cell, the
    expression of the fold (fold_kernels.hpp, k_fold_wave) evaluated in double.  cc: the float32 cross-correlation
    values of window_posterior; params: PARAM5_DTYPE [n]; sum_ref: the sums of the requests' particles [n]."""
    cc = np.asarray(cc, dtype=np.float64)
    params = np.asarray(params, dtype=PARAM5_DTYPE).reshape(-1)
    sumref = np.asarray(sum_ref, dtype=np.float64).reshape(-1)[:, None, None]
    assert cc.ndim == 3 and len(params) == len(cc) and sumref.shape[0] == len(cc)
    sumC = params["sumC"].astype(np.float64)[:, None, None]
    sumsqC = params["sumsquareC"].astype(np.float64)[:, None, None]
    Ntotpi = float(np.float32(int(N) * int(N)))
    with np.errstate(all="ignore"):
        d = sumC * sumC - sumsqC * Ntotpi
        norm = -(-sumC * sumref + Ntotpi * cc) / d
        mu = -(-sumC * cc + sumsqC * sumref) / d
    return norm, mu


def posterior_weights(requests, logp, log_prior=None, usable=None):
    """w float64 [n, nd, nd]: exp(logp + log_prior[orient]) normalised per particle over all cells of all its requests;
    0 where logp is not finite or `usable` (bool, logp's shape) is False; all 0 for a particle without a finite cell"""
    req = np.asarray(requests, dtype=WINDOW_REQUEST_DTYPE).reshape(-1)
    t = np.array(logp, dtype=np.float64)
    assert t.ndim == 3 and len(t) == len(req)
    if log_prior is not None:
        t = t + np.asarray(log_prior, dtype=np.float64)[req["orient"]][:, None, None]
    ok = np.isfinite(t)
    if usable is not None:
        ok &= np.asarray(usable, dtype=bool)
    t = np.where(ok, t, -np.inf)
    w = np.zeros_like(t)
    if len(req) == 0:
        return w
    p = req["particle"].astype(np.int64)
    nP = int(p.max()) + 1
    top = np.full(nP, -np.inf)
    np.maximum.at(top, p, t.reshape(len(t), -1).max(axis=1))
    live = np.isfinite(top[p])
    with np.errstate(invalid="ignore"):
        e = np.where(ok & live[:, None, None], np.exp(t - np.where(live, top[p], 0.0)[:, None, None]), 0.0)
    Z = np.zeros(nP)
    np.add.at(Z, p, e.reshape(len(e), -1).sum(axis=1))
    w[live] = e[live] / Z[p[live]][:, None, None]
    return w


def members(requests, group_of_request, logp, cc, params, sum_ref, N, weights=None, log_prior=None, want_weights=False):
    """(members SOFT_MEMBER_DTYPE [n], cells float64 [n, nd, nd]) for Engine.view_sums_soft, one member per request
    (particle, orient, conv) of WINDOW_REQUEST_DTYPE [n] in the group group_of_request[r].  logp, cc [n, nd, nd] and params
    [n]: window_posterior(want_cc, want_params) of the requests; sum_ref: float32 [nMaps] by particle; weights: float64
    [nMaps] by particle or None (1); log_prior: float64 by orientation or None.  want_weights: the posterior weights
    float64 [n, nd, nd] as a third value."""
    req = np.asarray(requests, dtype=WINDOW_REQUEST_DTYPE).reshape(-1)
    n = len(req)
    group = np.asarray(group_of_request, dtype=np.int32).reshape(-1)
    assert group.shape == (n,)
    p = req["particle"].astype(np.int64)
    norm, mu = cell_params(cc, params, np.asarray(sum_ref, dtype=np.float32)[p], N)
    w = posterior_weights(req, logp, log_prior, usable=np.isfinite(norm) & np.isfinite(mu))
    norm, mu = np.where(w > 0, norm, 0.0), np.where(w > 0, mu, 0.0)
    W = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)[p]
    out = np.zeros(n, dtype=SOFT_MEMBER_DTYPE)
    out["particle"], out["conv"] = req["particle"], req["conv"]
    cells = W[:, None, None] * (w * norm)
    out["s2"] = W * (w * norm * norm).reshape(n, -1).sum(axis=1)
    out["b"] = W * (w * norm * mu).reshape(n, -1).sum(axis=1)
    out["mass"] = W * w.reshape(n, -1).sum(axis=1)
    live = np.zeros(int(p.max()) + 1 if n else 0, dtype=bool)
    np.logical_or.at(live, p, w.reshape(n, -1).any(axis=1))
    out["group"] = np.where(live[p], group, -1) if n else group
    cells[out["group"] < 0] = 0.0
    return (out, cells, w) if want_weights else (out, cells)


def particle_summary(requests, w, nMaps):
    """PARTICLE_DTYPE [nMaps] from the posterior weights of the requests: requests per particle, n_eff = 1 / sum w^2 (0
    for a particle without weight) and the largest w"""
    req = np.asarray(requests, dtype=WINDOW_REQUEST_DTYPE).reshape(-1)
    out = np.zeros(int(nMaps), dtype=PARTICLE_DTYPE)
    out["particle"] = np.arange(int(nMaps))
    if len(req) == 0:
        return out
    p = req["particle"].astype(np.int64)
    flat = np.asarray(w, dtype=np.float64).reshape(len(req), -1)
    out["requests"] = np.bincount(p, minlength=int(nMaps))
    s2 = np.bincount(p, weights=(flat * flat).sum(axis=1), minlength=int(nMaps))
    out["n_eff"] = np.where(s2 > 0, 1.0 / np.where(s2 > 0, s2, 1.0), 0.0)
    np.maximum.at(out["mass_argmax"], p, flat.max(axis=1))
    return out


def _per_ctf(particle, orient, nCTF):
    n = len(particle)
    req = np.zeros(n * int(nCTF), dtype=WINDOW_REQUEST_DTYPE)
    req["particle"] = np.repeat(particle, nCTF)
    req["orient"] = np.repeat(orient, nCTF)
    req["conv"] = np.tile(np.arange(int(nCTF), dtype=np.int32), n)
    return req, req["orient"].astype(np.int32)


def requests_best(pmap, nCTF):
    """(requests WINDOW_REQUEST_DTYPE, group int32) for K = 1: every CTF set at the arg-max orientation of every particle
    a run compared (a record still as start_run left it, or with a negative orientation, has no request); particle-major,
    CTF sets ascending; group = orientation"""
    pmap = np.asarray(pmap)
    ok = ~((pmap["Total"] == 0.0) & (pmap["Constoadd"] == MIN_PROB)) & (pmap["orient"] >= 0)
    p = np.flatnonzero(ok).astype(np.int32)
    return _per_ctf(p, pmap["orient"][p].astype(np.int32), nCTF)


def requests_topk(candidates, K, nCTF):
    """(requests, group) for K >= 1: every CTF set at the first K candidates of every particle (CANDIDATE_DTYPE
    [nMaps, >= K], best first as topk_angles and the merged ranking deliver them; a candidate with a negative orientation
    is no candidate); particle-major, then rank, then CTF set; group = orientation"""
    cand = np.asarray(candidates)
    if cand.ndim != 2 or cand.shape[1] < int(K) or int(K) < 1:
        raise ValueError("requests_topk: %d candidates per particle for K = %d" % (cand.shape[-1] if cand.ndim == 2 else 0, K))
    o = cand["orient"][:, :int(K)].astype(np.int32)
    p = np.repeat(np.arange(len(cand), dtype=np.int32), int(K)).reshape(o.shape)
    keep = o >= 0
    return _per_ctf(p[keep], o[keep], nCTF)


def write(path, summary, sums, N, pixel_size):
    """appends the SOFT and SOFTSHELL lines to the --Reconstruct text file at path: summary PARTICLE_DTYPE [nMaps], sums =
    (weight, cross, powA, powB) of reconstruct.shell_sums of the two soft half-set spectra"""
    weight, cross, pa, pb = (np.asarray(x, dtype=np.float64) for x in sums)
    f, res, _, _ = _rc.derive(cross, pa, pb, N, pixel_size)
    with open(path, "a") as out:
        for r in np.asarray(summary, dtype=PARTICLE_DTYPE):
            out.write("SOFT %d %d %.15e %.15e\n" % (r["particle"], r["requests"], r["n_eff"], r["mass_argmax"]))
        for s in range(len(f)):
            out.write("SOFTSHELL %d %.15e %.15e %.15e %.15e %.15e %.15e\n" % (s, res[s], weight[s], f[s], cross[s], pa[s], pb[s]))


def parse(path):
    """(summary PARTICLE_DTYPE [nMaps], shells reconstruct.SHELL_DTYPE [nShells]) of the SOFT and SOFTSHELL lines of a
    --Reconstruct text file; the other lines are reconstruct.parse's.  Raises ValueError for a malformed SOFT line and for
    particles or shells out of order."""
    summary, shells = [], []
    with open(path) as f:
        for ln in f.read().split("\n"):
            t = ln.split()
            if not t or not t[0].startswith("SOFT"):
                continue
            if t[0] == "SOFT" and len(t) == 5:
                summary.append((int(t[1]), int(t[2]), float(t[3]), float(t[4])))
            elif t[0] == "SOFTSHELL" and len(t) == 8:
                shells.append((int(t[1]),) + tuple(float(x) for x in t[2:]))
            else:
                raise ValueError("%s: malformed line %r" % (path, ln))
    summary = np.array(summary, dtype=PARTICLE_DTYPE)
    shells = np.array(shells, dtype=_rc.SHELL_DTYPE)
    if (summary["particle"] != np.arange(len(summary))).any() or (shells["shell"] != np.arange(len(shells))).any():
        raise ValueError("%s: SOFT particles or SOFTSHELL shells out of order" % path)
    return summary, shells
