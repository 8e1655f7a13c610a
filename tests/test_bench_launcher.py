"""bench.py's own launcher (python bench.py --gpus N without torchrun): a rank that dies before or inside the
rendezvous must not leave the others waiting for the backend's timeout -- the parent watches every child, terminates
the rest on the first non-zero exit, keeps each rank's stderr in bench_rank<k>.err and returns the failed rank's code."""
import io
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD = r'''
import os, sys, time
rank = int(os.environ["RANK"])
assert os.environ["WORLD_SIZE"] == "3" and os.environ["MASTER_ADDR"] == "127.0.0.1" and int(os.environ["MASTER_PORT"]) > 0
if rank == 1:
    time.sleep(0.5)
    sys.stderr.write("rank 1: hipErrorNoDevice (stand-in failure)\n")
    sys.exit(3)
if rank == 0:
    print('{"partial": true}', flush=True)
time.sleep(120)          # stands for a rank waiting in the rendezvous / all-gather for the one that died
'''


def test_watchdog_terminates_the_other_ranks_and_reports_the_failed_one(tmp_path, monkeypatch, capsys):
    import bench
    monkeypatch.setenv("BIOEM_BENCH_LOGDIR", str(tmp_path))
    out = io.StringIO()
    t0 = time.time()
    rc = bench.self_launch(3, [sys.executable, "-c", CHILD], out=out)
    dt = time.time() - t0
    assert rc == 3 and dt < 10.0, (rc, dt)
    assert '"partial"' in out.getvalue()                        # rank 0's output is still handed through
    assert "hipErrorNoDevice" in open(tmp_path / "bench_rank1.err").read()
    err = capsys.readouterr().err
    assert "rank 1 of 3 exited with code 3" in err and "hipErrorNoDevice" in err
    for r in (0, 1, 2):
        assert os.path.exists(tmp_path / ("bench_rank%d.err" % r))


def test_launcher_returns_zero_and_rank0_output_when_all_ranks_succeed(tmp_path, monkeypatch):
    import bench
    monkeypatch.setenv("BIOEM_BENCH_LOGDIR", str(tmp_path))
    out = io.StringIO()
    rc = bench.self_launch(2, [sys.executable, "-c", "import os; print('line from rank', os.environ['RANK'])"], out=out)
    assert rc == 0 and out.getvalue() == "line from rank 0\n"


def test_bench_with_an_injected_rank_failure_returns_quickly(tmp_path):
    """The real script: rank 1 raises before the rendezvous (BIOEM_BENCH_INJECT_FAILURE=1).  On a box without a GPU
    rank 0 stops at its own "needs a GPU" check, so either rank may be reported first -- what is asserted is that the
    launch returns within seconds, non-zero, with the injected message in rank 1's file."""
    env = dict(os.environ, BIOEM_BENCH_LOGDIR=str(tmp_path), BIOEM_BENCH_INJECT_FAILURE="1", BIOEM_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0 and time.time() - t0 < 60
    assert "injected failure on rank 1" in open(tmp_path / "bench_rank1.err").read()
    assert "exited with code" in r.stderr


def test_config_selection_follows_baseline_json():
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8"]
        a = bench.parse_args()
        assert (a.particles, a.defocus, a.envelopes, a.orientations, a.pixels) == (10000, 2, 5, 4608, 224)   # config 3
        sys.argv = ["bench.py", "--gpus", "4"]
        a = bench.parse_args()
        assert (a.particles, a.defocus, a.envelopes, a.orientations) == (1000, 1, 5, 4608)                   # config 2
        sys.argv = ["bench.py", "--config", "3"]
        a = bench.parse_args()
        assert (a.gpus, a.particles, a.defocus) == (1, 10000, 2)
        sys.argv = ["bench.py", "--gpus", "8", "--config", "2", "--particles", "64"]
        a = bench.parse_args()
        assert (a.particles, a.defocus) == (64, 1)
    finally:
        sys.argv = argv


def test_time_budget_trims_warmup_first_then_steps():
    """--max-seconds: plan_steps is the pure function every rank evaluates with the same max-reduced numbers."""
    import bench
    # everything fits: nothing is trimmed
    assert bench.plan_steps(20, 4, 1.0, 30.0, 480.0, 10.0) == (4, 20)
    # config 3 on eight GPUs: 8.6 s per step, 60 s of set-up gone, 480 s budget, 10 s tail -> 47 steps fit: untouched
    assert bench.plan_steps(20, 4, 8.6, 60.0, 480.0, 10.0) == (4, 20)
    # a slower start: 200 s gone -> 31 fit -> 20 + 4 still fit
    assert bench.plan_steps(20, 4, 8.6, 200.0, 480.0, 10.0) == (4, 20)
    # 120 s budget: (120 - 40 - 10) / 8.6 = 8 steps fit: no further warm-up, eight timed steps
    assert bench.plan_steps(20, 4, 8.6, 40.0, 120.0, 10.0) == (0, 8)
    # warm-up is what goes first: 22 fit -> 2 of the 4 remaining warm-up steps, all 20 timed ones
    assert bench.plan_steps(20, 4, 1.0, 448.0, 480.0, 10.0) == (2, 20)
    # nothing fits any more: one timed step always runs (the line must exist), no warm-up
    assert bench.plan_steps(20, 4, 8.6, 500.0, 480.0, 10.0) == (0, 1)
    # no budget / no estimate: untouched
    assert bench.plan_steps(20, 4, 8.6, 500.0, 0.0, 10.0) == (4, 20)
    assert bench.plan_steps(20, 4, 0.0, 10.0, 480.0, 10.0) == (4, 20)


def test_shared_stack_path_is_per_launch_and_per_shape(monkeypatch):
    import bench
    monkeypatch.setenv("MASTER_PORT", "29511")
    a = bench.shared_stack_path((224, 10000, 4608, 5, 2))
    b = bench.shared_stack_path((224, 1000, 4608, 5, 1))
    assert a != b and a.startswith("/dev/shm/") and "29511" in a
    monkeypatch.setenv("MASTER_PORT", "29512")
    assert bench.shared_stack_path((224, 10000, 4608, 5, 2)) != a


def test_plain_run_keeps_its_step_count_and_full_restores_the_budget():
    """A plain run times exactly --steps steps (no wall-clock budget unless one is asked for); --full turns on the
    extra measurements and the 480 s budget."""
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse_args()
        assert (a.steps, a.warmup, a.full, a.max_seconds, a.dump_outputs) == (7, 2, False, 0.0, None)
        sys.argv = ["bench.py", "--full"]
        a = bench.parse_args()
        assert a.full and a.max_seconds == 480.0
        sys.argv = ["bench.py", "--max-seconds", "60", "--dump-outputs", "out"]
        a = bench.parse_args()
        assert (a.full, a.max_seconds, a.dump_outputs) == (False, 60.0, "out")
    finally:
        sys.argv = argv
    # no budget: plan_steps leaves both counts as asked
    assert bench.plan_steps(7, 1, 100.0, 1000.0, 0.0, 10.0) == (1, 7)


def _prob_block(n, seed=5):
    import numpy as np
    from bioem_amd.engine import CANDIDATE_DTYPE, PROB_MAP_DTYPE
    rng = np.random.default_rng(seed)
    pmap = np.zeros(n, dtype=PROB_MAP_DTYPE)
    for f in PROB_MAP_DTYPE.names:
        pmap[f] = rng.integers(-50, 50, size=n) if pmap[f].dtype.kind == "i" else rng.normal(size=n)
    cands = np.zeros((n, 3), dtype=CANDIDATE_DTYPE)
    for f in ("forAngles", "ConstAngle", "logp"):
        cands[f] = rng.normal(size=(n, 3))
    cands["orient"] = rng.integers(0, 4608, size=(n, 3))
    return pmap, cands


def test_dump_outputs_writes_every_field_as_float(tmp_path):
    import numpy as np
    import bench
    pmap, cands = _prob_block(100)
    names = bench.dump_outputs(str(tmp_path / "a"), pmap)
    assert names == sorted("map_" + f for f in pmap.dtype.names)
    for f in pmap.dtype.names:
        a = np.load(tmp_path / "a" / ("map_%s.npy" % f))
        assert a.dtype == (np.float32 if pmap[f].dtype == np.float32 else np.float64)
        assert np.array_equal(a, pmap[f])                       # exact: int32 and float fields alike
    names = bench.dump_outputs(str(tmp_path / "b"), pmap, cands)
    assert "angles_pad" not in names and "angles_orient" in names
    a = np.load(tmp_path / "b" / "angles_orient.npy")
    assert a.dtype == np.float64 and a.shape == (100, 3) and np.array_equal(a, cands["orient"])


def test_dump_outputs_samples_a_fixed_subset_above_the_limit(tmp_path):
    import numpy as np
    import bench
    pmap, cands = _prob_block(1000)
    limit = 20000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), pmap, cands, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "b")) == files and "particle_index.npy" in files
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in files) <= limit    # 128 = .npy header
    idx = np.load(tmp_path / "a" / "particle_index.npy").astype(np.int64)
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))      # same sample each time
    assert np.array_equal(np.load(tmp_path / "a" / "map_Total.npy"), pmap["Total"][idx])


def _run_bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    import json
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_and_full_runs_on_a_small_workload(tmp_path):
    """The plain line times exactly --steps steps and carries nothing of --full; the dumped outputs are the same in
    both runs (same seeded inputs); --full adds the CPU baseline, parity and the re-run check of the timed pass."""
    import numpy as np
    shape = ["--gpus", "1", "--particles", "20", "--orientations", "288"]
    plain = _run_bench(shape + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain")], 300)
    assert plain["steps"] == plain["steps_requested"] == 3 and plain["warmup"] == 1
    assert plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["unit"] == "comparisons/s"
    assert not {"cpu_baseline", "parity", "result_check"} & set(plain)
    full = _run_bench(shape + ["--steps", "2", "--warmup", "1", "--full", "--cpu-orientations", "8", "--cpu-repeats",
                               "1", "--dump-outputs", str(tmp_path / "full")], 300)
    assert full["result_check"]["ok"] and full["parity"]["argmax_mismatches"] == 0
    assert full["parity"]["max_rel_dlogp"] <= full["parity"]["tolerance_rel"] and full["cpu_baseline"]["value"] > 0
    names = plain["outputs"]["arrays"]
    assert names == full["outputs"]["arrays"] and "map_Total" in names and "map_orient" in names
    for n in names:
        a, b = np.load(tmp_path / "plain" / (n + ".npy")), np.load(tmp_path / "full" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == (20,) and np.array_equal(a, b), n
