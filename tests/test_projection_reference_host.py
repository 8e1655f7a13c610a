"""CPU tests of tests/projection_reference.py, the exact reference the GPU tests of the projection kernels compare with
(tests/test_projection_exact_gpu.py): against the real-space map of the oracle's orc_projection -- identical support,
identical count of skipped points, values within the oracle's float accumulation -- and against maps written out by hand
at the identity with one-Angstrom pixels: exact halves under floorf, the skip rules at the border, dist == rad2.

(A sphere always has irad = (int) (radius / px) + 1 >= 2, since radius > px: a footprint of irad 1 does not exist.  The
pixel sizes below give iradMax 2, 3 and 7, and 0 where every point is a single pixel.)"""
import math

import numpy as np
import pytest

import oracle as orc
import projection_reference as pr

f32 = np.float32


def oracle_map(points, NormDen, angle, is_quat, N, px, sx, sy):
    real = np.empty((N, N), dtype=f32)
    angle = np.ascontiguousarray(angle, dtype=f32)
    pts = np.ascontiguousarray(points)
    dropped = orc.lib().orc_projection(pts.ctypes.data, len(pts), f32(NormDen), angle.ctypes.data, int(is_quat), N,
                                       f32(px), sx, sy, real.ctypes.data, None)
    return real, dropped


def mixed_model(rng, n, extent):
    pts = pr.points_of(pr.ball(rng, n, extent), rng.uniform(1.2, 3.4, n), rng.uniform(0.5, 8.0, n))
    return pts


# px -> iradMax for radii 1.2 ... 3.4 A: 3.6 all points; 1.77 -> 2; 1.15 -> 3; 0.5 -> 7
CASES = [(64, 1.77, 2), (64, 1.15, 3), (64, 0.5, 7), (64, 3.6, 0), (35, 1.77, 2), (75, 1.15, 3)]


@pytest.mark.parametrize("N,px,irad_max", CASES)
@pytest.mark.parametrize("is_quat", [True, False])
@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-4, 5)])
def test_reference_against_the_oracle(N, px, irad_max, is_quat, shift):
    """support identical, skipped count identical, values within 2e-6 of the largest pixel (what
    test_device_projection_and_convolution grants the oracle's float sums); the model reaches past the border so that
    some points and spheres are skipped"""
    rng = np.random.default_rng(N * 1000 + int(px * 100) + 7 * is_quat + shift[0])
    pts = mixed_model(rng, 150, 0.52 * N * px)
    model = pr.Model(pts, N, px, *shift)
    assert model.iradMax == irad_max
    NormDen = 37.5
    angles = pr.unit_quaternions(rng, 6) if is_quat else pr.euler_angles(rng, 6)
    skipped_any = 0
    for a in angles:
        r = model.project(a, is_quat)
        real, dropped = oracle_map(pts, NormDen, a, is_quat, N, px, *shift)
        assert r.skipped == dropped
        skipped_any += dropped
        assert np.array_equal(r.exact != 0, real != 0)
        assert np.array_equal(r.n > 0, real != 0)          # (densities are positive: no term cancels)
        # the oracle scales by NormDen over its float tempden, whose accumulation alone is off by up to 3e-6 of the
        # value at a few thousand terms (one factor over the whole map); the reference restates that float sum
        tf = pr.float_tempden(r)
        assert abs(float(tf) - r.tempden) <= r.T * 2.0 ** -24 * r.tempden
        mine = r.exact * float(f32(NormDen) / tf)
        assert np.abs(mine - real).max() <= 2e-6 * np.abs(real).max()
        assert r.T == r.n.sum() and r.T > 0
        assert abs(r.exact.sum() - r.tempden) <= 1e-12 * r.tempden
        assert 0 <= r.edge_margin <= 0.5
    assert skipped_any > 0 and skipped_any < 6 * len(pts) // 2


def test_reference_takes_weights_from_a_stamp_table():
    rng = np.random.default_rng(5)
    pts = mixed_model(rng, 50, 20.0)
    a = pr.Model(pts, 64, 1.15)
    table = a.weight * 3.0
    table[~a.inside] = 123.0                                # outside the sphere the table is not read
    b = pr.Model(pts, 64, 1.15, stamps=table)
    q = pr.unit_quaternions(rng, 1)[0]
    ra, rb = a.project(q, True), b.project(q, True)
    assert np.array_equal(ra.n, rb.n)
    assert np.abs(rb.exact - 3.0 * ra.exact).max() <= 4 * 2.0 ** -53 * np.abs(rb.exact).max()


def test_fsum_per_pixel_is_exact_where_a_double_sum_is_not():
    """three points on one pixel, 1e16 + 1 - 1e16: a running double sum gives 0, the exact sum is 1"""
    pts = pr.points_of([[0, 0, 0]] * 3, 0.5, [1e16, 1.0, -1e16])
    r = pr.Model(pts, 8, 1.0).project(pr.IDENTITY, True)
    assert r.exact[4, 4] == 1.0 and r.n[4, 4] == 3 and abs(r.sabs[4, 4] - 2e16) < 1e10 and r.tempden == 1.0
    assert np.count_nonzero(r.exact) == 1




# ---- hand-made cases (projection_reference.hand_made_cases, the inputs the GPU tests use too): identity, px = 1; a
# point at pos lands on pixel floor(pos + N / 2 + 0.5) ----
HAND = {name: (N, pts, shift) for name, N, pts, shift in pr.hand_made_cases()}


def project_case(name):
    N, pts, shift = HAND[name]
    r = pr.Model(pts, N, 1.0, *shift).project(pr.IDENTITY, True)
    real, dropped = oracle_map(pts, 1.0, pr.IDENTITY, True, N, 1.0, *shift)
    assert dropped == r.skipped and np.array_equal(real != 0, r.exact != 0)
    return r


def test_floorf_on_exact_halves():
    """x + 8.5 is an integer for half-integer x: floorf keeps it (no round-half-even, no step down)"""
    r = project_case("exact_halves")                        # x = -0.5, 0.5, 1.5, -1.5, -2.5, 2.5 and y = x + 1
    want = np.zeros((16, 16))
    for i in [8, 9, 10, 7, 6, 11]:
        want[i, i + 1] = 1.0
    assert np.array_equal(r.exact, want)
    assert r.edge_margin == 0.0 and r.skipped == 0
    # and a float spacing of 8.5 below a half: the pixel before
    assert project_case("below_a_half").exact[8, 8] == 1.0


def test_points_at_the_border():
    """pixels -1 and N are skipped, 0 and N - 1 kept, on either axis; radius == px is still a point"""
    r = project_case("points_at_the_border")
    want = np.zeros((16, 16))
    want[0, 8] = want[15, 8] = want[8, 0] = want[8, 15] = 2.0
    assert np.array_equal(r.exact, want)
    assert r.skipped == 4 and r.tempden == 8.0 and r.T == 4


def disc(rows):
    return np.array([[ch == "#" for ch in row] for row in rows])


# radius 2 at px 1: irad 3, rad2 4, dist < 4 leaves di^2 + dj^2 in {0, 1, 2}: the 3 x 3 block ((2, 0) has dist == rad2)
DISC2 = disc(["###", "###", "###"])
# radius 5 at px 1: irad 6, rad2 25; (3, 4), (4, 3), (5, 0), (0, 5) have dist == rad2 and get no weight: 69 pixels
DISC5 = disc(["..#####..", ".#######.", "#########", "#########", "#########", "#########", "#########", ".#######.",
              "..#####.."])


def weight_by_hand(radius, d2, density):
    """the reference's weight for integer radius and px = 1, written out: float numerator, double division"""
    num = f32(f32(f32(f32(2) * np.sqrt(f32(radius * radius - d2))) * f32(density)) * f32(3))
    return float(num) / (4 * math.pi * radius * (radius * radius))


@pytest.mark.parametrize("name,radius,mask", [("radius_2_integral", 2, DISC2), ("radius_5_dist_equals_rad2", 5, DISC5)])
def test_integral_radius_and_dist_equal_rad2(name, radius, mask):
    Nn, c = 32, 16
    assert pr.Model(HAND[name][1], Nn, 1.0).iradMax == radius + 1
    r = project_case(name)
    h = mask.shape[0] // 2
    want = np.zeros((Nn, Nn))
    for di in range(-h, h + 1):
        for dj in range(-h, h + 1):
            if mask[di + h, dj + h]:
                want[c + di, c + dj] = weight_by_hand(radius, di * di + dj * dj, 1.5)
    assert np.count_nonzero(want) == (9 if radius == 2 else 69)
    assert np.array_equal(r.exact, want)
    for di, dj in ([(2, 0), (0, -2)] if radius == 2 else [(3, 4), (-4, 3), (5, 0), (0, -5)]):
        assert r.exact[c + di, c + dj] == 0.0 and r.n[c + di, c + dj] == 0


@pytest.mark.parametrize("shift", [(0, 0), (2, -1)])
def test_spheres_at_the_border(shift):
    """radius 2 (irad 3): centre pixels irad - 1 and N - irad are skipped, irad and N - irad - 1 kept, after the shift"""
    r = project_case("spheres_at_the_border_shift_%d_%d" % shift)   # centres (2, 3, 12, 13; 8) and (8; 2, 3, 12, 13)
    want = np.zeros((16, 16))
    for ci, cj in [(3, 8), (12, 8), (8, 3), (8, 12)]:
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                want[ci + di, cj + dj] += weight_by_hand(2, di * di + dj * dj, 1.0)
    assert np.array_equal(r.exact, want)
    assert r.skipped == 4 and r.T == 36
    i, j, keep = r.centres
    assert list(i[:4]) == [2, 3, 12, 13] and list(keep[:4]) == [False, True, True, False]


def test_shift_moves_spheres_only():
    r = project_case("shift_moves_spheres_only")           # a point at (8, 8), a sphere at (10, 10), shift (3, -2)
    assert r.exact[8, 8] == 1.0                              # the point stays
    assert r.exact[10 - 3, 10 + 2] == weight_by_hand(2, 0, 1.0) and r.exact[10, 10] == 0.0
