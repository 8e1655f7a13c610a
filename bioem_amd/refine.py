"""Orientation lists of a second, local round ("round 2" of the manual's model-comparison example, doc/index.rst
section modcom): every particle's best orientation of round 1 multiplied with a small grid of rotations.  numpy only,
no device; the lists go to Engine.upload_particle_orientations (one length) or upload_particle_orientation_lists (seed_lists:
as many seeds per particle as carry its round-1 posterior) and compare_own_orientations.

Quaternions are stored as the reference stores them, (x, y, z, w) with w = quat4 (bioem.cpp:1630-1646)."""
import numpy as np


def local_grid(n, step_rad):
    """(2n+1)^3 unit quaternions exp(step/2 * (i, j, k)), i, j, k in -n..n: rotations by step * |(i, j, k)| about the
    axis (i, j, k).  The identity comes FIRST, the others follow in (i, j, k) order; n = 2 gives the tutorial's 125.
    float64 [G, 4] in (x, y, z, w) order."""
    r = np.arange(-n, n + 1)
    ijk = np.array([(i, j, k) for i in r for j in r for k in r if (i, j, k) != (0, 0, 0)], dtype=np.float64)
    out = np.zeros((len(ijk) + 1, 4), dtype=np.float64)
    out[0, 3] = 1.0
    if len(ijk):
        v = 0.5 * float(step_rad) * ijk  # half angle x axis
        half = np.linalg.norm(v, axis=1)
        out[1:, :3] = v * (np.sin(half) / half)[:, None]
        out[1:, 3] = np.cos(half)
    return out


def hamilton(a, b):
    """Hamilton product a (x) b of quaternions in (x, y, z, w) storage, broadcasting over leading axes; float64."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def compose(best, grid):
    """best[nMaps, 4] x grid[G, 4] -> float32 [nMaps, G, 4]: the Hamilton product best (x) grid, normalised.

    The order of the product is THIS project's convention (the tutorial's multiply_quat.py is not part of the reference
    tree).  With M(q) the matrix the reference builds from a stored quaternion (bioem.cpp:1638-1646; it is the
    transpose of the textbook matrix of q), M(best (x) grid) = M(grid) M(best): the model is rotated by `best` first,
    and the small rotation of the grid then acts on the rotated model, in the frame of the image.  An entry whose grid
    quaternion is the identity (0, 0, 0, 1) is `best` itself, bit for bit."""
    best = np.asarray(best)
    grid = np.asarray(grid)
    assert best.ndim == 2 and best.shape[1] == 4 and grid.ndim == 2 and grid.shape[1] == 4
    q = hamilton(best[:, None, :], grid[None, :, :])
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    out = q.astype(np.float32)
    ident = np.all(grid == np.array([0.0, 0.0, 0.0, 1.0]), axis=1)
    out[:, ident, :] = np.asarray(best, dtype=np.float32)[:, None, :]
    return np.ascontiguousarray(out)


def refine_lists(angles, pmap, grid):
    """The per-particle lists of round 2 from a round-1 result: angles[nAngles, 4] is the round-1 quaternion list,
    pmap its probability block (pmap["orient"][p] = best orientation of particle p)."""
    angles = np.asarray(angles)
    return compose(angles[np.asarray(pmap["orient"], dtype=np.int64)], grid)


def seed_lists(angles, cands, grid, max_seeds=1, log_window=np.inf):
    """Round-2 lists around SEVERAL round-1 orientations per particle: a sharp particle needs one seed, an ambiguous one
    the few that carry its posterior.

    angles[nAngles, 4]: the round-1 quaternion list; cands[nMaps][K]: the candidates of Engine.topk_angles (fields
    "orient", "logp"), best first, orient = -1 beyond the owned count.  Particle p keeps at most max_seeds seeds in
    candidate order: always the first, then those with logp >= logp_first - log_window.  Its list is the concatenation
    of compose(seed, grid) over its seeds (no duplicate removal), so entry 0 of every seed's block is the seed itself
    where the grid's first entry is the identity.  Returns (flat float32 [n, 4], offsets int64 [nMaps + 1])."""
    angles = np.asarray(angles)
    grid = np.asarray(grid)
    assert max_seeds >= 1 and log_window >= 0
    G = len(grid)
    parts, offsets = [], [0]
    for row in cands:
        orient = np.asarray(row["orient"], dtype=np.int64)
        logp = np.asarray(row["logp"], dtype=np.float64)
        seeds = []
        first = None
        for o, l in zip(orient, logp):
            if o < 0:
                continue
            if first is None:
                first = l
            elif not l >= first - log_window:
                continue
            seeds.append(int(o))
            if len(seeds) == max_seeds:
                break
        if seeds:
            parts.append(compose(angles[seeds], grid).reshape(len(seeds) * G, 4))
        offsets.append(offsets[-1] + len(seeds) * G)
    flat = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), dtype=np.float32)
    return np.ascontiguousarray(flat, dtype=np.float32), np.asarray(offsets, dtype=np.int64)
