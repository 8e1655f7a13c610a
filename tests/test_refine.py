"""bioem_amd.refine (the lists of a second, local round) and the command line's --RefineOrientations refusals: no GPU."""
import math
import os
import subprocess

import numpy as np

from bioem_amd import refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.array([0.0, 0.0, 0.0, 1.0])


def ref_matrix(q):
    """the matrix the reference builds from a stored quaternion (x, y, z, w), in ITS index order (bioem.cpp:1638-1646);
    the rotated point is sum_j rotmat[k][j] pos[j] (bioem.cpp:1690)"""
    q0, q1, q2, q3 = [float(v) for v in q]
    m = np.zeros((3, 3))
    m[0][0] = 1 - 2 * q1 * q1 - 2 * q2 * q2
    m[1][0] = 2 * (q0 * q1 - q2 * q3)
    m[2][0] = 2 * (q0 * q2 + q1 * q3)
    m[0][1] = 2 * (q0 * q1 + q2 * q3)
    m[1][1] = 1 - 2 * q0 * q0 - 2 * q2 * q2
    m[2][1] = 2 * (q1 * q2 - q0 * q3)
    m[0][2] = 2 * (q0 * q2 - q1 * q3)
    m[1][2] = 2 * (q1 * q2 + q0 * q3)
    m[2][2] = 1 - 2 * q0 * q0 - 2 * q1 * q1
    return m


def random_unit(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1)[:, None]).astype(np.float32)


def test_local_grid_is_unit_identity_first_and_sized_like_the_tutorial():
    for n, count in ((0, 1), (1, 27), (2, 125)):
        g = refine.local_grid(n, math.radians(4.0))
        assert g.shape == (count, 4)
        assert np.array_equal(g[0], IDENT)
        assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max() < 1e-15
        assert len({tuple(np.round(r, 12)) for r in g}) == count  # all different
    # entry (i, j, k) is the rotation by step |(i, j, k)| about (i, j, k)
    g = refine.local_grid(1, 0.1)
    ang = 2.0 * np.arccos(g[1:, 3])
    assert np.allclose(sorted(set(np.round(ang, 12))), [0.1, 0.1 * math.sqrt(2), 0.1 * math.sqrt(3)])


def test_compose_is_unit_float32_and_keeps_best_under_the_identity():
    best = random_unit(9, 1)
    grid = refine.local_grid(1, math.radians(4.0))
    out = refine.compose(best, grid)
    assert out.dtype == np.float32 and out.shape == (9, 27, 4) and out.flags["C_CONTIGUOUS"]
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=2) - 1.0).max() < 2e-7
    assert refine.compose(best, IDENT[None]).tobytes() == best[:, None, :].tobytes()  # bitwise
    assert out[:, 0].tobytes() == best.tobytes()
    # a 4 degree step moves the orientation by 4 ... 4 sqrt(3) degrees
    dots = np.abs(np.sum(out[:, 1:].astype(np.float64) * best[:, None, :], axis=2))
    rot = np.degrees(2.0 * np.arccos(np.clip(dots, -1, 1)))
    assert rot.min() > 3.99 and rot.max() < 4.0 * math.sqrt(3) + 0.01


def test_compose_order_against_the_reference_rotation_matrices():
    """Pins which matrix product best (x) grid is: M(best (x) grid) == M(grid) M(best) with the reference's own
    matrices -- the model is rotated by `best` first, the grid's small rotation acts on the result -- and NOT
    M(best) M(grid)."""
    best = random_unit(5, 2)
    grid = refine.local_grid(1, math.radians(10.0))[1:]
    out = refine.compose(best, grid)
    worst_other = 0.0
    for i in range(len(best)):
        for k in range(len(grid)):
            m = ref_matrix(out[i, k])
            assert np.abs(m - ref_matrix(grid[k]) @ ref_matrix(best[i])).max() < 5e-6
            worst_other = max(worst_other, np.abs(m - ref_matrix(best[i]) @ ref_matrix(grid[k])).max())
    assert worst_other > 1e-2  # the two orders differ for these rotations: the test can tell them apart
    # in words: a model point x goes to M(grid) (M(best) x)
    x = np.array([3.0, -1.0, 2.0])
    assert np.allclose(ref_matrix(out[0, 0]) @ x, ref_matrix(grid[0]) @ (ref_matrix(best[0]) @ x), atol=1e-4)


def test_refine_lists_takes_every_particles_best_orientation():
    angles = random_unit(40, 3)
    pmap = np.zeros(6, dtype=[("orient", "<i4")])
    pmap["orient"] = [3, 39, 0, 3, 17, 8]
    grid = refine.local_grid(2, math.radians(2.0))
    lists = refine.refine_lists(angles, pmap, grid)
    assert lists.shape == (6, 125, 4)
    assert np.array_equal(lists[:, 0], angles[pmap["orient"]])
    assert np.array_equal(lists, refine.compose(angles[pmap["orient"]], grid))


def _cli(tmp_path, param_text, extra):
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    assert os.path.exists(exe), "CLI not built"
    (tmp_path / "param.txt").write_text(param_text)
    (tmp_path / "grid.txt").write_text("1\n" + "".join("%11.8f " % v for v in IDENT) + "\n")
    cmd = [exe, "--Inputfile", "param.txt", "--Modelfile", "none.txt", "--Particlesfile", "none.txt",
           "--RefineOrientations", "grid.txt"] + extra
    return subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


BASE = "PIXEL_SIZE 2.2\nNUMBER_PIXELS 64\nCTF_B_ENV 20.0 200.0 3\nCTF_DEFOCUS 1.0 3.0 2\nCTF_AMPLITUDE 0.1 0.1 1\n" \
       "DISPLACE_CENTER 6 1\n"


def test_cli_refuses_refinement_it_cannot_do_before_it_needs_a_device(tmp_path):
    """Euler angles, PRIOR_ANGLES and WRITE_PROB_ANGLES are refused right after the parameter file is read: no particle,
    model or device has been touched (the model and particle files of these runs do not exist)."""
    r = _cli(tmp_path, BASE + "GRIDPOINTS_ALPHA 4\nGRIDPOINTS_BETA 2\n", [])
    assert r.returncode == 1 and "Error - --RefineOrientations needs quaternions" in r.stdout
    r = _cli(tmp_path, BASE + "USE_QUATERNIONS\nPRIOR_ANGLES\n", ["--ReadOrientation", "grid.txt"])
    assert r.returncode == 1 and "Error - --RefineOrientations is not valid with prior for orientations" in r.stdout
    r = _cli(tmp_path, BASE + "USE_QUATERNIONS\nGRIDPOINTS_QUATERNION 2\nWRITE_PROB_ANGLES 3\n", [])
    assert r.returncode == 1 and "Error - --RefineOrientations is not valid with WRITE_PROB_ANGLES" in r.stdout
    # without the option the same parameter file gets past that point: it stops at the particle file
    (tmp_path / "param.txt").write_text(BASE + "USE_QUATERNIONS\nGRIDPOINTS_QUATERNION 2\nWRITE_PROB_ANGLES 3\n")
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    r = subprocess.run([exe, "--Inputfile", "param.txt", "--Modelfile", "none.txt", "--Particlesfile", "none.txt"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 1 and "RefineOrientations" not in r.stdout


def test_cli_reads_the_refinement_list_with_the_options(tmp_path):
    """a missing or malformed list ends the run before particles, model or a device are touched, not after round 1"""
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    (tmp_path / "param.txt").write_text(BASE + "USE_QUATERNIONS\nGRIDPOINTS_QUATERNION 2\n")
    (tmp_path / "short.txt").write_text("3\n" + "".join("%11.8f " % v for v in IDENT) + "\n")
    (tmp_path / "range.txt").write_text("1\n" + "".join("%11.8f " % v for v in (0.0, 0.0, 0.0, 1.5)) + "\n")
    for name, msg in (("absent.txt", "Quaterion list file"), ("short.txt", "Less quaternions than expected"),
                      ("range.txt", "Value out of range")):
        r = subprocess.run([exe, "--Inputfile", "param.txt", "--Modelfile", "none.txt", "--Particlesfile", "none.txt",
                            "--RefineOrientations", name], cwd=str(tmp_path), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode == 1 and msg in r.stdout, r.stdout[-500:]


def test_cli_usage_names_the_option():
    exe = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
    r = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert "--RefineOrientations" in r.stdout
