"""GPU tests of the projection kernels alone (k_project, k_project_stamps, k_project_coords + k_project_bands, k_project_box
and the boxed double-input r2c behind them) against the exact reference of tests/projection_reference.py, through
Engine.debug_projection_maps / Engine.debug_stamps.

Per pixel: |got - exact| <= (n + 1) 2^-53 sum|term| with n the number of terms the pixel receives -- n double additions in
any order -- and a pixel without a term is exactly 0.0; tempden within (T + 16) 2^-53 sum|term|.  One misplaced, dropped or
doubled item fails this.  Paths 1 (box) and 2 (bands) read their weights from the footprint table, so the reference is
handed the device's own table for them (test_stamps_bit_for_bit checks that table on its own); path 3 (global atomics)
computes the weights inline and is compared with the reference's.

A sphere has irad = (int) (radius / px) + 1 >= 2 because radius > px: where a case list asks for a footprint of irad 1, the
smallest that exists, 2, stands in.

Handles of one particle and one CTF set: maxOrientations grows to the orientation count (2 048 at most)."""
import numpy as np
import pytest

import projection_reference as pr

pytestmark = pytest.mark.gpu

f32 = np.float32
NORM_DEN = 37.5
PATHS = {1: "box", 2: "bands", 3: "atomics"}


def make_engine(N, pts, px, angles, is_quat=True, shift=(0, 0)):
    import bioem_amd.engine as eng
    pd = eng.ParamDevice()
    pd.maxDisplaceCenter, pd.GridSpaceCenter, pd.NumberPixels, pd.NumberFFTPixels1D = 2, 1, N, N // 2 + 1
    pd.NxDisp, pd.NtotDisp, pd.Ntotpi, pd.volu = 5, 25, float(N * N), 1.0
    pd.sigmaPriorbctf, pd.sigmaPriordefo, pd.Priordefcent, pd.sigmaPrioramp, pd.Priorampcent = 100.0, 2.0, 3.0, 0.5, 0.0
    angles = np.ascontiguousarray(angles, dtype=f32).reshape(-1, 4)
    E = eng.Engine(pd, 1, len(angles), 1, algo=1, device=0)
    E.upload_model(pts, NORM_DEN, px, *shift)
    E.upload_orientations(angles, is_quat)
    assert E.max_batch()[0] == min(len(angles), 2048)
    return E


class Case:
    """a model, a list and the engine that holds them; the reference models are built once"""

    def __init__(self, N, pts, px, angles, is_quat=True, shift=(0, 0)):
        self.N, self.pts, self.px, self.is_quat, self.shift = N, pts, px, is_quat, shift
        self.angles = np.ascontiguousarray(angles, dtype=f32).reshape(-1, 4)
        self.E = make_engine(N, pts, px, self.angles, is_quat, shift)
        self._models, self._results = {}, {}
        self.worst = [0.0, 0.0]                 # largest achieved fraction of the pixel and the tempden bound

    def close(self):
        print("achieved fraction of the bound: pixel %.3f, tempden %.3f" % tuple(self.worst))
        self.E.close()

    def reference(self, own_stamps, o):
        if own_stamps not in self._models:
            stamps = self.E.debug_stamps()[0] if own_stamps else None
            self._models[own_stamps] = pr.Model(self.pts, self.N, self.px, *self.shift, stamps=stamps)
        if (own_stamps, o) not in self._results:
            self._results[own_stamps, o] = self._models[own_stamps].project(self.angles[o], self.is_quat)
        return self._results[own_stamps, o]

    def check(self, path, want_path=None, o0=0, nO=None):
        """every pixel of every orientation [o0, o0 + nO) under this path against the exact map; returns info"""
        nO = len(self.angles) - o0 if nO is None else nO
        maps, td, _, info = self.E.debug_projection_maps(o0, nO, PATHS.get(path, path))
        assert info["path"] == (want_path if want_path is not None else path), info
        for b in range(nO):
            r = self.reference(info["path"] != 3, o0 + b)
            bound = pr.pixel_bound(r)
            err = np.abs(maps[b] - r.exact)
            bad = np.argwhere(~(err <= bound))
            assert len(bad) == 0, (path, o0 + b, bad[:5], maps[b][tuple(bad[0])], r.exact[tuple(bad[0])])
            assert not maps[b][r.n == 0].any()             # exactly 0.0 where no term lands
            tb = pr.tempden_bound(r)
            assert abs(td[b] - r.tempden) <= tb, (path, o0 + b, td[b], r.tempden, tb)
            with np.errstate(all="ignore"):
                frac = np.where(bound > 0, err / bound, 0.0).max()
            self.worst[0] = max(self.worst[0], float(frac))
            self.worst[1] = max(self.worst[1], abs(td[b] - r.tempden) / tb if tb > 0 else 0.0)
        return info

    def refused(self, path, match):
        """the forced path is refused with 2 and a message, and the handle still projects"""
        with pytest.raises(RuntimeError, match=match) as ei:
            self.E.debug_projection_maps(0, 1, PATHS[path])
        assert ei.value.rc == 2
        self.E.debug_projection_maps(0, 1, "auto")


def mixed_points(rng, n, extent, radii, lo=-2.0, hi=8.0):
    """n points in a ball; radii drawn from the list; densities in [lo, hi) with one exact zero and one negative"""
    pts = pr.points_of(pr.ball(rng, n, extent), rng.choice(np.asarray(radii, dtype=f32), n), rng.uniform(lo, hi, n))
    if n >= 3:
        pts["density"][n // 3] = 0.0
        pts["density"][n // 2] = -1.25
    return pts


# ---- (a) the footprint table ----
STAMP_RADII_PX1 = [0.5, 1.0,                                # radius <= px: a point, its stamp all zero
                   float(np.nextafter(f32(1), f32(2))), 1.01,   # just above px: irad 2, the centre and its 4 neighbours
                   1.5, 2.5, 4.5, 6.5, 15.5,                # irad 2, 3, 5, 7, 16
                   5.0,                                     # dist == rad2 at (3, 4) and (5, 0)
                   2.0, 3.0, 4.0]                           # radius / px integral


@pytest.mark.parametrize("px", [1.0, 1.77])
def test_stamps_bit_for_bit(px):
    """k_project_stamps against the reference's weights: the same bits (float chain of the numerator with a correctly
    rounded sqrtf, double division), 0.0 outside the sphere and outside the point's own irad"""
    rng = np.random.default_rng(11)
    if px == 1.0:
        radius = np.array(STAMP_RADII_PX1, dtype=f32)
        density = np.array([1.0, 2.0, 1.0, 3.5, -2.0, 0.0, 1.0, 0.37, 1.0, 1.5, 1.0, 7.25, 0.5], dtype=f32)
    else:
        radius = (rng.uniform(0.5, 9.0, 60) * px).astype(f32)
        density = rng.uniform(-2.0, 8.0, 60).astype(f32)
    pts = pr.points_of(np.zeros((len(radius), 3)), radius, density)
    E = make_engine(64, pts, px, pr.IDENTITY)
    try:
        got, irad_max = E.debug_stamps()
        inside, weight, irad, R = pr.footprint_tables(pts, px)
        assert irad_max == R and got.shape == weight.shape
        if px == 1.0:
            assert R == 16 and sorted(set(irad.tolist())) == [0, 2, 3, 4, 5, 6, 7, 16]
            assert not got[0].any() and not got[1].any()
            assert np.count_nonzero(got[2]) == 5 and np.count_nonzero(got[9]) == 69
        assert not got[~inside].any()
        assert got.tobytes() == weight.tobytes(), np.argwhere(got != weight)[:5]
    finally:
        E.close()


def test_no_stamps_beyond_33_pixels():
    """irad 17: no footprint table; paths 1 and 2 are refused and a run takes k_project"""
    rng = np.random.default_rng(12)
    pts = mixed_points(rng, 12, 10.0, [0.7, 2.5, 16.5])
    pts["radius"][0] = 16.5
    c = Case(96, pts, 1.0, pr.unit_quaternions(rng, 3))
    try:
        with pytest.raises(RuntimeError, match="no footprint table") as ei:
            c.E.debug_stamps()
        assert ei.value.rc == 2
        c.refused(1, "no footprint table")
        c.refused(2, "no footprint table")
        info = c.check(0, want_path=3)
        assert info["iradMax"] == 17
        c.check(3)
    finally:
        c.close()


# ---- (b) every path against the exact map ----
@pytest.mark.parametrize("nPts", [1, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4100])
def test_record_list_edges(nPts):
    """k_project_bands loads 2 048 records per round, lists them 512 at a time, 256 per load, and clamps the ragged tail;
    k_project_box and k_project walk the same points in strides of 512 and blocks of 256.  The model stays inside the
    map, so every record of a group reaches the (single, 64-row) band and a list fills to its 512 entries.  At 4 100
    points the records no longer fit the row-pass buffer of a 64-pixel image (2 112): the band path is refused there."""
    rng = np.random.default_rng(nPts)
    pts = mixed_points(rng, nPts, 7.0, [0.6, 0.9, 1.5, 1.9, 2.5])
    c = Case(64, pts, 1.0, pr.unit_quaternions(rng, 3))
    try:
        info = c.check(0, want_path=1)
        assert info["TR"] == 80 and info["compact"] == 1
        c.check(1)
        if nPts <= 2112:
            c.check(2)
        else:
            c.refused(2, "do not fit")
        c.check(3)
    finally:
        c.close()


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_grid_stride_of_the_box_kernel():
    """3 nCU + 5 orientations from o0 = 3: the resident grid of 3 nCU blocks takes a second trip for five of them"""
    rng = np.random.default_rng(21)
    nO = 3 * compute_units() + 5
    pts = mixed_points(rng, 7, 9.0, [0.6, 1.5, 2.5])
    c = Case(64, pts, 1.0, pr.unit_quaternions(rng, nO + 3))
    try:
        c.check(1, o0=3, nO=nO)
        c.check(0, want_path=1, o0=3, nO=nO)
    finally:
        c.close()


def test_grid_stride_of_the_band_kernel():
    """N = 128: bands of 40, 40, 40 and 8 rows; more (orientation, band) units than the 3 nCU resident blocks"""
    rng = np.random.default_rng(22)
    nO = 3 * compute_units() // 4 + 2
    assert nO * 4 > 3 * compute_units()
    pts = mixed_points(rng, 24, 50.0, [0.6, 1.5, 2.5, 3.5])
    c = Case(128, pts, 1.0, pr.unit_quaternions(rng, nO + 3))
    try:
        info = c.check(2, o0=3, nO=nO)
        assert info["TR"] == 40
        c.check(0, want_path=2, o0=3, nO=nO)        # (the box of this model has 111 pixels a side: 96 KiB)
        c.refused(1, "52 KiB")
    finally:
        c.close()


@pytest.mark.parametrize("N,TR", [(128, 40), (200, 25), (426, 12)])
def test_band_boundaries(N, TR):
    """identity, px = 1: for every boundary r0 between two bands, centres on every row r0 - irad - 1 ... r0 + irad + 1 with
    irad 0 (points), 2 and 3 (the list filter i + irad >= r0 && i - irad < r1 and the clamp of the rows a band takes),
    each in a column of its own neighbourhood; the last band is ragged at 128 (8 rows) and 426 (6 rows).  (The rows
    +-irad of a footprint never carry weight -- irad px > radius --, so only the points see the filter's last row.)"""
    pos, radius = [], []
    col = 8
    for r0 in range(TR, N, TR):
        for irad, rad in ((0, 0.7), (2, 1.5), (3, 2.5)):
            for row in range(r0 - irad - 1, r0 + irad + 2):
                if irad <= row < N - irad:
                    pos.append([row - N / 2, col - N / 2, 0])
                    radius.append(rad)
                    col = 8 + (col - 8 + 5) % (N - 16)
    pts = pr.points_of(pos, radius, np.linspace(0.5, 3.0, len(pos)))
    c = Case(N, pts, 1.0, np.stack([pr.IDENTITY, pr.z_rotation(90)]))
    try:
        r = c.reference(False, 0)
        assert r.skipped == 0 and r.edge_margin == 0.5
        info = c.check(2)
        assert info["TR"] == TR
        c.check(0, want_path=2)
        c.check(3)
        c.refused(1, "52 KiB")
    finally:
        c.close()


def test_bands_of_fewer_than_twelve_rows_are_refused():
    """N = 427: TR = 11; the band path is refused and a run takes k_project"""
    rng = np.random.default_rng(23)
    pts = mixed_points(rng, 40, 200.0, [0.6, 1.5, 2.5])
    c = Case(427, pts, 1.0, pr.unit_quaternions(rng, 2))
    try:
        c.refused(2, "fewer than 12 rows")
        info = c.check(0, want_path=3)
        assert info["TR"] == 11
    finally:
        c.close()


def test_mixed_footprints():
    """irad 0 (points), 2, 3, 5, 7 and 16 in one model: S = 33, seven fetch groups of five stamp entries in the box
    kernel, and points whose own irad is smaller skip columns"""
    rng = np.random.default_rng(24)
    pts = mixed_points(rng, 60, 18.0, [0.8, 1.5, 2.5, 4.5, 6.5, 15.5])
    pts["radius"][:6] = [0.8, 1.5, 2.5, 4.5, 6.5, 15.5]
    c = Case(96, pts, 1.0, pr.unit_quaternions(rng, 5))
    try:
        info = c.check(0, want_path=1)
        assert info["iradMax"] == 16 and info["boxSide"] <= 81
        assert c.reference(True, 0).skipped == 0
        c.check(1)
        c.check(2)
        c.check(3)
    finally:
        c.close()


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-4, 5)])
def test_model_reaching_past_the_map(shift):
    """N = 48, the model wider than the map: points and spheres are skipped at the border by the reference's rules, the
    box is the whole map by its clamps"""
    rng = np.random.default_rng(25)
    pts = mixed_points(rng, 200, 27.0, [0.6, 1.5, 2.5, 3.5])
    c = Case(48, pts, 1.0, pr.unit_quaternions(rng, 4), shift=shift)
    try:
        assert all(0 < c.reference(False, o).skipped < 100 for o in range(4))
        info = c.check(1)
        assert info["boxLo"] == 0 and info["boxSide"] == 48
        c.check(0, want_path=1)
        c.check(2)
        c.check(3)
    finally:
        c.close()


@pytest.mark.parametrize("name,N,pts,shift", pr.hand_made_cases(), ids=[x[0] for x in pr.hand_made_cases()])
def test_hand_made_border_cases(name, N, pts, shift):
    """the cases of tests/test_projection_reference_host.py (expected maps written out there): exact halves under floorf,
    points at -1 / 0 / N - 1 / N, spheres at irad - 1 / irad / N - irad - 1 / N - irad, dist == rad2"""
    c = Case(N, pts, 1.0, pr.IDENTITY, shift=shift)
    try:
        c.check(0, want_path=1)
        c.check(1)
        c.check(2)
        c.check(3)
    finally:
        c.close()


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-4, 5), (5, 5), (-5, -5)])
def test_box_margin(shift):
    """the farthest point of the model, a sphere of iradMax, is turned onto +-x, +-y and the diagonals (its coordinate an
    exact half pixel, so that floorf sits on its edge); nothing the reference keeps is missing, and the box the host
    sized holds the reference's support"""
    pts = pr.points_of([[25.5, 0, 0], [0, -25.5, 0], [3, 4, 5], [-2, 1, 0], [18, 18, 0]], [6.5, 6.5, 0.7, 2.5, 6.5],
                       [1.0, 2.0, 3.0, -1.0, 1.0])
    angles = np.stack([pr.z_rotation(d) for d in (0, 90, 180, 270, 45, 135, 225, 315)])
    c = Case(96, pts, 1.0, angles, shift=shift)
    try:
        info = c.check(1)
        lo, hi = info["boxLo"], info["boxLo"] + info["boxSide"] - 1
        for o in range(len(angles)):
            r = c.reference(True, o)
            assert r.skipped == 0
            rows, cols = np.nonzero(r.n)
            assert lo <= min(rows.min(), cols.min()) and max(rows.max(), cols.max()) <= hi
        c.check(0, want_path=1)
    finally:
        c.close()


def euler_safe_model(rng, n, extent, radii, N, px, angles):
    """points whose coordinates before floorf stay >= 1e-3 pixel away from an integer in every orientation of the list:
    the device's cosf / sinf may differ from the host's in the last bits, which moves a coordinate by ~1e-5 pixel at a
    reach of 30; points that violate the margin are drawn again, on the host, before anything is uploaded"""
    pts = mixed_points(rng, n, extent, radii)
    redrawn = 0
    for _ in range(100):
        m = pr.Model(pts, N, px)
        margin = np.full(n, 1.0)
        for a in angles:
            c = m.pixels(a, False)[2].astype(np.float64)
            margin = np.minimum(margin, np.abs(c - np.rint(c)).min(axis=1))
        bad = np.nonzero(margin < 1e-3)[0]
        if len(bad) == 0:
            break
        redrawn += len(bad)
        pts["pos"][bad] = pr.ball(rng, len(bad), extent)
    assert len(bad) == 0 and redrawn < 0.2 * n, redrawn
    return pts


def test_euler_lists():
    rng = np.random.default_rng(26)
    angles = pr.euler_angles(rng, 16)
    pts = euler_safe_model(rng, 200, 30.0, [0.6, 1.5, 2.5], 96, 1.0, angles)
    c = Case(96, pts, 1.0, angles, is_quat=False)
    try:
        assert min(c.reference(False, o).edge_margin for o in range(16)) >= 1e-3
        c.check(0, want_path=1)
        c.check(1)
        c.check(2)
        c.check(3)
    finally:
        c.close()


def test_quaternions_that_stretch_the_model():
    """|q| = 1.07: the reference's matrix is no rotation, the model may leave its box; a run takes the bands, the box is
    refused"""
    rng = np.random.default_rng(27)
    pts = mixed_points(rng, 150, 14.0, [0.6, 1.5, 2.5])
    angles = (pr.unit_quaternions(rng, 4) * f32(1.07)).astype(f32)
    c = Case(64, pts, 1.0, angles)
    try:
        c.check(0, want_path=2)
        c.refused(1, "unit length")
        c.check(2)
        c.check(3)
    finally:
        c.close()


def test_invalid_arguments_are_refused():
    rng = np.random.default_rng(28)
    c = Case(64, mixed_points(rng, 10, 8.0, [0.6, 1.5]), 1.0, pr.unit_quaternions(rng, 5))
    try:
        for args in [(0, 6, 0), (0, 0, 0), (-1, 2, 0), (4, 2, 0), (0, 1, 4), (0, 1, -1)]:
            with pytest.raises(RuntimeError) as ei:
                c.E.debug_projection_maps(*args)
            assert ei.value.rc == 2
        c.check(0, want_path=1)
    finally:
        c.close()


# ---- (c) the r2c from double maps ----
def scaled_maps(maps, td):
    """what the transform behind the projection is given: the double map scaled by NormDen / tempden in float
    (bioem.cpp:1808-1818)"""
    ratio = f32(NORM_DEN) / td.astype(f32)
    img = maps.astype(f32) * ratio[:, None, None]
    assert img.dtype == f32
    return img


def spectrum_from_maps(maps, td):
    """... transformed in double"""
    return np.fft.rfft2(scaled_maps(maps, td).astype(np.float64))


def check_spectrum(c, path="auto"):
    import os
    import r2c_reference as rr
    maps, td, spec, info = c.E.debug_projection_maps(0, len(c.angles), path, want_spec=True)
    want = spectrum_from_maps(maps, td)
    got = spec[..., 0].astype(np.float64) + 1j * spec[..., 1]
    assert np.abs(got - want).max() <= 1.5e-7 * np.abs(want).max()
    # word by word against the exact transform of the same float images (tests/r2c_reference.py)
    img = scaled_maps(maps, td)
    re, im = rr.exact_r2c(img)
    m = rr.m_of(c.N, os.environ.get("BIOEM_R2C") == "dft")
    v = rr.verdict(spec, re, im, np.abs(img.astype(np.float64)).sum(axis=(1, 2)), m)
    print("N %d box [%d, +%d): m %d  %s" % (c.N, info["boxLo"], info["boxSide"], m, v))
    assert v.bad == 0 and v.share <= 1.0, (str(v), v.first_bad)
    return spec, info


R2C_BOXES = {
    # name: (N, extent of the model in pixels, radii, shift, what info must show)
    "odd_side": (64, 10.0, [0.6, 2.5], (0, 0), lambda i, N: i["compact"] and i["boxSide"] % 2 == 1 and i["boxLo"] > 0),
    "even_side": (64, 10.0, [0.6, 2.5], (1, 0), lambda i, N: i["compact"] and i["boxSide"] % 2 == 0 and i["boxLo"] > 0),
    "side_3": (64, 0.0, [0.6], (0, 0), lambda i, N: i["compact"] and i["boxSide"] == 3),
    "lo_0": (64, 20.0, [0.6, 1.5], (9, 9), lambda i, N: i["compact"] and i["boxLo"] == 0 and i["boxSide"] < N),
    "whole_map": (64, 30.0, [0.6, 1.5], (0, 0), lambda i, N: i["compact"] and i["boxLo"] == 0 and i["boxSide"] == N),
    "odd_n35": (35, 8.0, [0.6, 1.5], (0, 0), lambda i, N: i["compact"] and 0 < i["boxSide"] < N),
    "mfma_n46": (46, 8.0, [0.6, 1.5], (0, 0), lambda i, N: not i["compact"]),
    "prime_n47": (47, 8.0, [0.6, 1.5], (0, 0), lambda i, N: not i["compact"]),
}


def r2c_case(name, seed=31):
    N, extent, radii, shift, _ = R2C_BOXES[name]
    rng = np.random.default_rng(seed)
    n = 1 if extent == 0.0 else 40
    pts = pr.points_of(pr.ball(rng, n, extent), rng.choice(np.asarray(radii, dtype=f32), n), rng.uniform(0.5, 4.0, n))
    if extent:
        pts["pos"][0] = [extent, 0, 0]                      # modelRadius is the extent
    return Case(N, pts, 1.0, pr.unit_quaternions(rng, 7), shift=shift)


@pytest.mark.parametrize("name", sorted(R2C_BOXES))
def test_r2c_from_the_double_maps(name, monkeypatch):
    """the spectrum against a double transform of the device's own maps: compact boxes of odd and even side (rows go in
    pairs, an odd side pairs its last row with itself), of 3 pixels, at the map's edge, the whole map; 7 orientations so
    that row pairs run over image boundaries; sizes without the fast transform store whole maps"""
    monkeypatch.delenv("BIOEM_R2C", raising=False)
    c = r2c_case(name)
    try:
        spec, info = check_spectrum(c)
        assert info["path"] == 1 and R2C_BOXES[name][4](info, c.N), info
        c.check(0, want_path=1)
        if name in ("odd_side", "lo_0"):                    # whole maps from the other kernels through the same transform
            check_spectrum(c, "bands")
            check_spectrum(c, "atomics")
    finally:
        c.close()


@pytest.mark.parametrize("N", [64, 100])
def test_exact_dft_from_the_double_maps(N, monkeypatch):
    """BIOEM_R2C=dft: the box kernel stores the whole map and the exact-DFT kernels transform it; the same rounded
    values as the fast transform but for a few last-bit flips (at most 2 % of the words)"""
    rng = np.random.default_rng(N)
    pts = pr.points_of(pr.ball(rng, 40, 12.0), rng.choice(np.asarray([0.6, 1.5, 2.5], dtype=f32), 40),
                       rng.uniform(0.5, 4.0, 40))
    c = Case(N, pts, 1.0, pr.unit_quaternions(rng, 7))
    try:
        monkeypatch.delenv("BIOEM_R2C", raising=False)
        fast, info = check_spectrum(c)
        assert info["compact"] == 1
        monkeypatch.setenv("BIOEM_R2C", "dft")
        slow, info = check_spectrum(c)
        assert info["path"] == 1 and info["compact"] == 0
        c.check(0, want_path=1)
        differ = np.count_nonzero(fast != slow)
        assert differ <= 0.02 * fast.size, differ
    finally:
        c.close()
