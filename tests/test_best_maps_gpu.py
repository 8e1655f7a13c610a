"""GPU tests of bioem_hip_render_best_maps (Engine.render_best_maps): the calculated image of a best-match record,

    out[(k + X) mod N][(j + Y) mod N] = conv[k][j] / N^2 * norm + mu,   conv = c2r(P_o conj(CTF_c)) unnormalised,

against the oracle chain  norm * roll(irfft2_float64(orc.convolve(orc.projection(...), refCTF[c])[0]), (X, Y)) + mu.
Expected values never come from the code under test.  Tolerances: 1e-4 relative to the map's scale for the whole chain
(the project's end-to-end figure against the oracle), 2e-6 of the map's maximum for the transform alone fed with the
device's own spectrum (the figure granted to a device spectrum in test_gpu_parity.py)."""
import os

import numpy as np
import pytest

import oracle as orc
from golden_util import load_case, oracle_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_TOL = 1e-4
TRANSFORM_TOL = 2e-6
GOLDEN_OF_SIZE = {32: "g3_n32_trace", 35: "g9_n35_odd", 48: "g1_n48", 64: "g10_n64", 224: "g7_n224"}
NORMS = [1.0, -0.37, 2.5e3]
MUS = [0.0, -4.25]


class Scene:
    """model, orientation list and CTF kernels of a size: a golden case where there is one, else a synthetic workload;
    an engine on it that holds nRec particles' worth of records and no particles"""

    def __init__(self, N=None, nRec=14, golden=None, algo=1, synthetic=False, nOrient=6, maxD=5):
        import bioem_amd.engine as eng
        golden = golden or (None if synthetic else GOLDEN_OF_SIZE.get(N))
        if golden:
            S = oracle_setup(load_case(golden))
            self.N, self.points, self.NormDen, self.px = S.N, S.points, S.NormDen, S.px
            self.angles, self.isQuat, self.refCTF, self.ctfParam = S.angles, S.isQuat, S.refCTF, S.ctfParam
            self.shift = (S.P["shiftX"], S.P["shiftY"])
            self.maxD = S.pd.maxDisplaceCenter
            pd = eng.ParamDevice()
            for f, _ in eng.ParamDevice._fields_:
                setattr(pd, f, getattr(S.pd, f))
        else:
            from bioem_amd.synthetic import Workload
            W = Workload(N=N, nP=1, nOrient=nOrient, nEnv=2, maxD=maxD, render=False)
            W.engine.close()
            self.N, self.points, self.NormDen, self.px = N, W.points, W.NormDen, W.px
            self.angles, self.isQuat, self.refCTF, self.ctfParam = W.angles, True, W.refCTF, W.ctfParam
            self.shift = (0, 0)
            self.maxD = maxD
            pd = W.pd
        self.pd = pd
        self.nA, self.nCTF = len(self.angles), len(self.refCTF)
        self.nRec = nRec
        self.engine = self.make_engine(nRec, algo)
        self._img = {}

    def make_engine(self, nMaps, algo=1, orientations=True, **kw):
        import bioem_amd.engine as eng
        E = eng.Engine(self.pd, nMaps, self.nA, self.nCTF, algo=algo, device=0, **kw)
        E.upload_ctf(self.refCTF, self.ctfParam)
        E.upload_model(self.points, self.NormDen, self.px, *self.shift)
        if orientations:
            E.upload_orientations(self.angles, self.isQuat)
        return E

    def image(self, angle, c):
        """irfft2 in float64 of the oracle's conv spectrum: conv / N^2"""
        key = (tuple(np.asarray(angle, dtype=np.float32).tolist()), int(c))
        if key not in self._img:
            N = self.N
            spec = orc.projection(self.points, self.NormDen, angle, self.isQuat, N, self.px, *self.shift)
            conv = orc.convolve(spec, self.refCTF[c])[0]
            z = conv[..., 0].astype(np.float64) + 1j * conv[..., 1].astype(np.float64)
            self._img[key] = np.fft.irfft2(z, s=(N, N))
        return self._img[key]

    def expected(self, rec, angle=None):
        img = self.image(self.angles[rec["orient"]] if angle is None else angle, rec["conv"])
        want = float(rec["norm"]) * np.roll(img, (int(rec["cent_x"]), int(rec["cent_y"])), axis=(0, 1)) + float(rec["mu"])
        return want, abs(float(rec["norm"])) * np.abs(img).max() + abs(float(rec["mu"]))

    def records(self, n=None):
        """hand-made records: every shift of the set on both axes, mixed within a batch; every CTF; first and last
        orientation; every norm and offset"""
        import bioem_amd.engine as eng
        n = self.nRec if n is None else n
        N = self.N
        shifts = [0, 1, -1, self.maxD, -self.maxD, N - 1, -(N - 1)]
        rec = np.zeros(n, dtype=eng.PROB_MAP_DTYPE)
        for i in range(n):
            rec[i]["cent_x"] = shifts[i % 7]
            rec[i]["cent_y"] = shifts[(3 * i + 2) % 7]
            rec[i]["conv"] = i % self.nCTF
            rec[i]["orient"] = [0, self.nA - 1, self.nA // 2][i % 3]
            rec[i]["norm"] = NORMS[(i // 2) % 3]
            rec[i]["mu"] = MUS[i % 2]
        return rec

    def check(self, got, rec, angles=None, what=""):
        worst = 0.0
        for i, r in enumerate(rec):
            want, scale = self.expected(r, None if angles is None else angles[i])
            ratio = np.abs(got[i] - want).max() / scale
            worst = max(worst, ratio)
            assert ratio <= CHAIN_TOL, (what, i, ratio, r)
        print("%s N=%d: max |delta| / scale = %.3g (bound %g)" % (what, self.N, worst, CHAIN_TOL))


_scenes = {}


def scene(N):
    if N not in _scenes:
        nCTFmin = 4 if N == 224 else 14
        _scenes[N] = Scene(N, nRec=nCTFmin)
        if N != 224 and _scenes[N].nCTF > 14:
            _scenes[N].engine.close()
            _scenes[N] = Scene(N, nRec=_scenes[N].nCTF)
    return _scenes[N]


SIZES = [32, 35, 37, 48, 64, 224]


@pytest.mark.parametrize("N", SIZES)
def test_kernel_cells_against_the_oracle(N):
    """(a) hand-made records, no run: even, odd, prime (A = 1), 64 with the Nyquist column, 224 with 4 records"""
    sc = scene(N)
    rec = sc.records()
    if N != 224:
        assert set(rec["conv"]) == set(range(sc.nCTF)) and {0, sc.nA - 1} <= set(rec["orient"])
        assert {0, 1, -1, sc.maxD, -sc.maxD, N - 1, 1 - N} <= set(rec["cent_x"]) | set(rec["cent_y"])
    got = sc.engine.render_best_maps(rec)
    assert got.shape == (len(rec), N, N) and got.dtype == np.float32
    sc.check(got, rec, what="cells")


@pytest.mark.parametrize("N", SIZES)
def test_transform_alone_on_the_device_spectrum(N):
    """(b) the two inverse passes fed with the device's own conv spectrum: float64 irfft2 of debug_convolution(o, c)
    against the render with norm 1, offset 0, no shift"""
    import bioem_amd.engine as eng
    sc = scene(N)
    E = sc.engine
    worst = 0.0
    for o, c in [(0, 0), (sc.nA - 1, sc.nCTF - 1)]:
        spec, _, _ = E.debug_convolution(o, c)
        want = np.fft.irfft2(spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64), s=(N, N))
        rec = np.zeros(sc.nRec, dtype=eng.PROB_MAP_DTYPE)
        rec["orient"], rec["conv"], rec["norm"] = o, c, 1.0
        got = E.render_best_maps(rec, 0, 1)[0]
        ratio = np.abs(got - want).max() / np.abs(want).max()
        worst = max(worst, ratio)
        print("transform N=%d (o=%d, c=%d): max |delta| / max |map| = %.3g (bound %g)" % (N, o, c, ratio, TRANSFORM_TOL))
    assert worst <= TRANSFORM_TOL


def test_psf_kernel_conjugate_sign():
    """(c) a complex (PSF) kernel: the sign of the conjugate in Z = P conj(CTF)"""
    sc = Scene(golden="g13_n32_psf_writectf")
    assert np.abs(sc.refCTF[..., 1]).max() > 0
    rec = sc.records()
    sc.check(sc.engine.render_best_maps(rec), rec, what="psf")
    sc.engine.close()


def test_batch_boundaries_bit_identical():
    """(d) N = 32, nMaps = maxOrientations + 3: two batches with a ragged last one, a sub-range across the boundary.  Every
    map equals the one-particle call's, bit for bit; a repeated call gives the same bytes"""
    sc = Scene(32, nRec=9, synthetic=True)
    E = sc.engine
    maxO = E.max_batch()[0]
    assert sc.nRec == maxO + 3
    rec = sc.records()
    full = E.render_best_maps(rec)
    assert full.tobytes() == E.render_best_maps(rec).tobytes()
    sub = E.render_best_maps(rec, 5, maxO + 1)
    assert sub.shape[0] == maxO - 4
    for p in range(sc.nRec):
        one = E.render_best_maps(rec, p, p + 1)
        assert one.tobytes() == full[p].tobytes(), p
        if 5 <= p < maxO + 1:
            assert one.tobytes() == sub[p - 5].tobytes(), p
    sc.check(full, rec, what="batches")
    E.close()


def test_own_lists():
    """(e) ragged own lists (1, 4, 0, 7, ...): records index the particle's own list; the particle with the empty list is
    refused inside the range, a range without it succeeds"""
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import random_quaternions
    sc = Scene(32, nRec=8, synthetic=True, nOrient=7)
    E = sc.engine
    lengths = [1, 4, 0, 7, 2, 5, 3, 6]
    assert max(lengths) <= sc.nA
    pool = random_quaternions(sum(lengths), seed=77)
    lists, k = [], 0
    for n in lengths:
        lists.append(pool[k:k + n])
        k += n
    rec = sc.records()
    for p, n in enumerate(lengths):
        rec[p]["orient"] = [0, n - 1, n // 2][p % 3] if n else 0
    with pytest.raises(RuntimeError) as e:
        E.render_best_maps(rec, own=True)
    assert e.value.rc == 2 and "lists" in str(e.value)
    E.upload_particle_orientation_lists(lists, True)
    with pytest.raises(RuntimeError, match="particle 2") as e:
        E.render_best_maps(rec, own=True)
    assert e.value.rc == 2
    lo = E.render_best_maps(rec, 0, 2, own=True)
    hi = E.render_best_maps(rec, 3, 8, own=True)
    angles = [lists[p][rec[p]["orient"]] for p in (0, 1, 3, 4, 5, 6, 7)]
    sc.check(np.concatenate([lo, hi]), rec[[0, 1, 3, 4, 5, 6, 7]], angles=angles, what="own lists")
    E.close()


def test_refused_records_leave_the_handle_usable():
    """(f) every refusal returns 2 with a message, and a valid call still succeeds afterwards"""
    sc = scene(32)
    E = sc.engine
    good = sc.records()
    ref = E.render_best_maps(good).tobytes()

    def refused(rec, *a, **kw):
        with pytest.raises(RuntimeError) as e:
            E.render_best_maps(rec, *a, **kw)
        assert e.value.rc == 2, str(e.value)
        assert E.render_best_maps(good).tobytes() == ref
        return str(e.value)

    for field, value in (("orient", sc.nA), ("orient", -1), ("conv", sc.nCTF), ("cent_x", sc.N), ("cent_y", -sc.N)):
        bad = good.copy()
        bad[3][field] = value
        assert "particle 3" in refused(bad)
        assert len(E.render_best_maps(bad, 4, sc.nRec)) == sc.nRec - 4   # (a range that leaves the record out)
    refused(good, 5, 2)
    refused(good, 4, 4)
    refused(good, 0, sc.nRec + 1)
    refused(good, own=True)
    # nothing uploaded: model, CTFs, orientations
    import bioem_amd.engine as eng
    E2 = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)
    for step in (lambda: E2.upload_model(sc.points, sc.NormDen, sc.px, *sc.shift),
                 lambda: E2.upload_ctf(sc.refCTF, sc.ctfParam),
                 lambda: E2.upload_orientations(sc.angles, sc.isQuat)):
        with pytest.raises(RuntimeError, match="not uploaded") as e:
            E2.render_best_maps(good)
        assert e.value.rc == 2
        step()
    assert E2.render_best_maps(good).tobytes() == ref
    E2.close()


def test_every_handle_kind_and_both_algos(monkeypatch):
    """shard handles, BIOEM_CC_DIRECT handles and ALGO 2 render the same bytes as the plain ALGO-1 handle; a tiled
    wide window (no kernel covers it in one piece) renders against the oracle"""
    sc = scene(32)
    rec = sc.records()
    ref = sc.engine.render_best_maps(rec).tobytes()
    for kw in (dict(algo=2), dict(shard=(2, 4))):
        E = sc.make_engine(sc.nRec, **kw)
        assert E.render_best_maps(rec).tobytes() == ref, kw
        E.close()
    monkeypatch.setenv("BIOEM_CC_DIRECT", "1")
    E = sc.make_engine(sc.nRec)
    assert E.kernel_signature.startswith("k_compare_direct")
    assert E.render_best_maps(rec).tobytes() == ref
    E.close()
    monkeypatch.delenv("BIOEM_CC_DIRECT")
    tiled = Scene(42, nRec=7, synthetic=True, maxD=16)
    import ctypes as C
    sig = C.create_string_buffer(256)
    assert tiled.engine.L.bioem_hip_plan(42, 16, 1, 1, sig, 256) == 0 and b" tiles of " in sig.value
    rec = tiled.records()
    tiled.check(tiled.engine.render_best_maps(rec), rec, what="tiled window")
    tiled.engine.close()


def test_end_to_end_render_is_the_fit_of_the_particle():
    """(g) the convention, end to end: particles planted at 1e-3 noise with shifts up to +-8, one pass, finish_run,
    render.  The render of a particle whose record is the planted (orientation, CTF, shift) is the least-squares fit of
    that particle: rms(particle - render) <= 1e-2 rms(particle), ten times the planted noise.  The same render with the
    shift's sign flipped misses that bound wherever the shift is not zero."""
    import bioem_amd.engine as eng
    from bioem_amd.synthetic import Workload
    W = Workload(N=64, nP=16, nOrient=32, nEnv=2, maxD=10, snr=1e6)
    E = W.engine
    raw, pmap, _ = eng.new_prob_block(W.nP, W.nOrient, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, W.nOrient)
    E.finish_run(raw)
    maps = E.render_best_maps(pmap)
    kept = flipped = 0
    for p in range(W.nP):
        sx, sy = np.random.default_rng(20260102 + p).integers(-8, 9, size=2)   # synthetic.Workload.render_particles
        planted = ((7919 * p) % W.nOrient, p % W.nCTF, int(sx), int(sy))
        r = pmap[p]
        if (r["orient"], r["conv"], r["cent_x"], r["cent_y"]) != planted:
            print("particle %d left out: record %s, planted %s" % (p, r, planted))
            continue
        kept += 1
        part = W.maps[p].astype(np.float64)
        rms = np.sqrt(np.mean(part ** 2))
        res = np.sqrt(np.mean((part - maps[p]) ** 2))
        print("particle %d shift (%d, %d): rms residual / rms particle = %.3g" % (p, sx, sy, res / rms))
        assert res <= 1e-2 * rms, (p, res / rms)
        if sx or sy:
            wrong = np.roll(maps[p].astype(np.float64), (-2 * int(sx), -2 * int(sy)), axis=(0, 1))
            assert np.sqrt(np.mean((part - wrong) ** 2)) > 1e-2 * rms, p
            flipped += 1
    assert kept >= 0.9 * W.nP
    assert flipped > 0
    E.close()


# ------------------------------------------------------------------------------------------------------
# (h) command line: --BestMaps, --PrintBestCalMap
# ------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "bioem_amd", "bin", "bioEM")
CLI_CASE = "g10_n64"


def run_cli(args, cwd, **env):
    import subprocess
    r = subprocess.run([EXE] + args, cwd=str(cwd), env=dict(os.environ, BIOEM_GPUS="1", **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout


def read_stack(path):
    """MRC mode-2 stack -> maps [nz][N][N] as the --ReadMRC reader lays them out (sections transposed)"""
    import struct
    raw = open(path, "rb").read()
    nx, ny, nz, mode = struct.unpack("<4i", raw[:16])
    assert mode == 2 and struct.unpack("<i", raw[92:96])[0] == 0 and len(raw) == 1024 + 4 * nx * ny * nz
    return np.frombuffer(raw, dtype="<f4", offset=1024).reshape(nz, ny, nx).transpose(0, 2, 1)


def test_cli_best_maps_stack(tmp_path):
    """--BestMaps on a golden case: Output_Probabilities is byte-identical to a run without the option, the stack holds
    the maps Engine.render_best_maps gives for the same records (the run repeated here on the host layer's own set-up of
    the same files), one shard or three; with --RefineOrientations the round-1 file is unchanged and FILE_Round2
    appears"""
    import bioem_amd.engine as eng
    from bioem_amd import hostlib, refine
    from golden_util import write_case_inputs
    case = load_case(CLI_CASE)
    assert case["model_format"] == "text" and case["particles"] == "text"
    d = tmp_path
    param = os.path.join(case["dir"], "param.txt")
    inputs = ["--Inputfile", param] + write_case_inputs(case, d)
    run_cli(inputs + ["--OutputFile", "plain.txt"], d, BIOEM_ALGO="1")
    run_cli(inputs + ["--OutputFile", "out.txt", "--BestMaps", "best.mrc"], d, BIOEM_ALGO="1")
    assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    stack = read_stack(d / "best.mrc")
    S, angles, ref, par = hostlib.setup_from_files(param, str(d / "orient.txt") if case["orient_lines"] else None)
    pts, nd = hostlib.read_model(str(d / "model.txt"), nocentermass=bool(S.nocentermass), pixelSize=S.pixelSize)
    maps = hostlib.read_particles(str(d / "particles.txt"), S.pd.NumberPixels)
    assert stack.shape == maps.shape
    E = eng.Engine(S.pd, len(maps), S.nAngles, S.nCTF, algo=1, device=0)
    E.upload_particle_maps(maps)
    E.upload_ctf(ref, par)
    E.upload_model(pts, nd, S.pixelSize, S.shiftX, S.shiftY)
    E.upload_orientations(angles, S.isQuat)
    raw, pmap, _ = eng.new_prob_block(len(maps), S.nAngles, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    want = E.render_best_maps(pmap)
    E.close()
    assert np.array_equal(stack, want)
    run_cli(inputs + ["--OutputFile", "out3.txt", "--BestMaps", "best3.mrc"], d, BIOEM_ALGO="1", BIOEM_SHARDS="3")
    assert open(d / "out3.txt", "rb").read() == open(d / "plain.txt", "rb").read()
    assert np.array_equal(read_stack(d / "best3.mrc"), want)
    if S.isQuat:
        q = refine.local_grid(1, 0.05)
        with open(d / "grid.txt", "w") as f:
            f.write("%d\n" % len(q) + "".join("".join("%11.8f " % float(v) for v in r) + "\n" for r in q))
        run_cli(inputs + ["--OutputFile", "r.txt", "--RefineOrientations", "grid.txt", "--BestMaps", "bestr.mrc"], d,
                BIOEM_ALGO="1")
        assert open(d / "r.txt", "rb").read() == open(d / "plain.txt", "rb").read()
        assert np.array_equal(read_stack(d / "bestr.mrc"), want)
        second = read_stack(d / "bestr.mrc_Round2")
        assert second.shape == want.shape and np.isfinite(second).all() and np.abs(second).max() > 0


def best_file_and_oracle_map(case, rec, extra=""):
    """a BEST_* file from one parsed line of Output_Probabilities, and the oracle's unshifted map norm * conv / N^2 + mu
    for exactly the numbers of that file"""
    import ctypes as C
    P = case["P"]
    assert not P["usepsf"] and not P["nocentermass"]
    N, px = P["N"], P["pixelSize"]
    quat = len(rec["angles"]) == 4
    keys = ["BEST_Q1", "BEST_Q2", "BEST_Q3", "BEST_Q4"] if quat else ["BEST_ALPHA", "BEST_BETA", "BEST_GAMMA"]
    text = "PIXEL_SIZE %r\nNUMBER_PIXELS %d\n" % (float(px), N) + ("USE_QUATERNIONS\n" if quat else "")
    text += "".join("%s %r\n" % (k, v) for k, v in zip(keys, rec["angles"]))
    amp, defocus, env = rec["ctf"]
    text += "BEST_CTF_AMP %r\nBEST_CTF_DEFOCUS %r\nBEST_CTF_B_ENV %r\n" % (amp, defocus, env)
    text += "BEST_DX %d\nBEST_DY %d\nBEST_NORM %r\nBEST_OFFSET %r\n" % (rec["cx"], rec["cy"], rec["norm"], rec["mu"])
    text += "SHIFT_X %d\nSHIFT_Y %d\n" % (P["shiftX"], P["shiftY"]) + extra
    f32 = np.float32
    phase = f32(defocus * np.pi * 2.0 * 10000 * float(f32(0.019866)))
    g = orc.CtfGrid(f32(amp), f32(amp), 1, phase, phase, 1, f32(env), f32(env), 1)
    ctf = np.zeros((1, N, N // 2 + 1, 2), dtype=f32)
    par, steps = np.zeros((1, 3), dtype=f32), np.zeros(3, dtype=f32)
    vp = C.c_void_p
    assert orc.lib().orc_ctf_kernels(N, f32(px), 0, C.byref(g), ctf.ctypes.data_as(vp), par.ctypes.data_as(vp),
                                     steps.ctypes.data_as(vp)) == 1
    points, NormDen = orc.model_from_array(case["model"], False)
    angle = np.zeros(4, dtype=f32)
    angle[:len(rec["angles"])] = rec["angles"]
    spec = orc.projection(points, NormDen, angle, quat, N, px, P["shiftX"], P["shiftY"])
    conv = orc.convolve(spec, ctf[0])[0]
    img = np.fft.irfft2(conv[..., 0].astype(np.float64) + 1j * conv[..., 1].astype(np.float64), s=(N, N))
    return text, rec["norm"] * img + rec["mu"], abs(rec["norm"]) * np.abs(img).max() + abs(rec["mu"])


def parse_bestmap(text, N, ddx, ddy):
    """BESTMAP text -> (MAP values [N][N], list of MAPddx (k, j, printed value))"""
    v = np.full((N, N), np.nan)
    printed = {}
    shifted = []
    for ln in text.split("\n"):
        t = ln.split()
        if not t:
            continue
        if t[0] == "MAP":
            k, j = int(t[1]) - ddx, int(t[2]) - ddy
            v[k, j] = float(t[3])
            printed[(k, j)] = t[3]
        else:
            assert t[0] == "MAPddx", ln
            shifted.append((int(t[1]), int(t[2]), t[3]))
    return v, printed, shifted


def test_cli_print_best_cal_map(tmp_path):
    """--PrintBestCalMap on a BEST_* file made from one line of a golden Output_Probabilities: the MAP lines parse to the
    oracle's map within the chain tolerance plus half a unit of the sixth printed digit; the MAPddx lines obey the rule.
    WITHNOISE 0.5 at 64^2: the residual against the noise-free file has a sample deviation within 10 % of 0.5 (standard
    error 1.1 % at 4 096 samples), MAP lines only, and two runs in different seconds differ."""
    import time

    import io_formats as iof
    from golden_util import golden_output
    case = load_case(CLI_CASE)
    d = tmp_path
    iof.write_text_model(str(d / "model.txt"), case["model"])
    recs = iof.parse_output_probabilities(golden_output(case, 1))
    rec = next((r for r in recs if r["cx"] or r["cy"]), recs[0])
    N, ddx, ddy = case["P"]["N"], rec["cx"], rec["cy"]
    text, want, scale = best_file_and_oracle_map(case, rec)
    (d / "best.txt").write_text(text)
    out = run_cli(["--Modelfile", "model.txt", "--PrintBestCalMap", "best.txt"], d)
    assert "Best map printed in file: BESTMAP" in out
    clean_text = open(d / "BESTMAP").read()
    got, printed, shifted = parse_bestmap(clean_text, N, ddx, ddy)
    assert not np.isnan(got).any()
    digit = 0.5 * 10.0 ** (np.floor(np.log10(np.maximum(np.abs(want), 1e-300))) - 5)
    excess = np.abs(got - want) - digit
    print("BESTMAP: max (|delta| - half digit) / scale = %.3g (bound %g)" % (excess.max() / scale, CHAIN_TOL))
    assert (excess <= CHAIN_TOL * scale).all()
    expect = [(k, j) for k in range(N) for j in range(N)
              if k + ddx < N and j + ddy < N and 0 <= k - ddx < N and 0 <= j - ddy < N]
    assert [(k, j) for k, j, _ in shifted] == expect
    assert all(s == printed[(k - ddx, j - ddy)] for k, j, s in shifted)
    assert clean_text.count(" \n") == N
    # noise
    (d / "noisy.txt").write_text(text + "WITHNOISE 0.5\n")
    run_cli(["--Modelfile", "model.txt", "--PrintBestCalMap", "noisy.txt"], d)
    first = open(d / "BESTMAP").read()
    t0 = int(time.time())            # (taken AFTER the run: a run that crosses into the next second was seeded with either)
    while int(time.time()) == t0:    # (the generator is seeded with the second, like the reference's)
        time.sleep(0.05)
    run_cli(["--Modelfile", "model.txt", "--PrintBestCalMap", "noisy.txt"], d)
    second = open(d / "BESTMAP").read()
    assert first != second
    a, _, sa = parse_bestmap(first, N, ddx, ddy)
    assert not sa and not np.isnan(a).any()
    sd = np.std(a - got, ddof=1)
    print("WITHNOISE 0.5: sample deviation of the residual %.4f" % sd)
    assert abs(sd - 0.5) <= 0.05
