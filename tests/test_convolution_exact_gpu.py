"""GPU tests of the convolution kernels alone (k_convolve + k_parseval_ordered, k_convolve_sums<4, 4 | 3, 5 | 3, 6>, and
k_unreorder behind every debug read-back) slot by slot against tests/convolution_reference.py, through
Engine.debug_convolve_batch: whole batches (nO, c0, nC) launched as a run launches them.

Class A (integer spectra with planted bins of 2^25, exact whatever is fused): spectrum, sumC, sumsquareC and amp / pha / env
of every slot bit for bit.  Class B (rounded values): every component within 2 * 2^-24 (|a b| + |c d|) of the exact product,
sumC the bits of conv[0][0].re, sumsquareC within (M + 3) 2^-24 relative of the exact weighted sum over the device's own
spectrum.  Every batch: no word of its rows left unwritten, the guard row and guard parameters untouched, the raw bytes
equal to the comparison layout stated in Python.

One handle per image size, 13 CTF sets, 16 orientations (208 conv rows per batch: 7 x 13 and a guard row fit)."""
import ctypes

import numpy as np
import pytest

import convolution_reference as cr

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
U = 2.0 ** -24
N_ANGLES = 16
_engines = {}


def engine_of(N):
    if N not in _engines:
        import bioem_amd.engine as eng
        pd = eng.ParamDevice()
        pd.maxDisplaceCenter, pd.GridSpaceCenter, pd.NumberPixels, pd.NumberFFTPixels1D = 2, 1, N, N // 2 + 1
        pd.NxDisp, pd.NtotDisp, pd.Ntotpi, pd.volu = 5, 25, float(N * N), 1.0
        pd.sigmaPriorbctf, pd.sigmaPriordefo, pd.Priordefcent, pd.sigmaPrioramp, pd.Priorampcent = 100.0, 2.0, 3.0, 0.5, 0.0
        E = eng.Engine(pd, 1, N_ANGLES, cr.N_CTF, algo=1, device=0)
        assert E.max_batch() == (N_ANGLES, N_ANGLES * cr.N_CTF)
        _engines[N] = E
    return _engines[N]


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for E in _engines.values():
        E.close()
    _engines.clear()


def run_batch(E, data, shape, fused, monkeypatch):
    """one launch shape: (conv [rows, N, H, 2], params [rows], info), the coverage, guard and raw-layout assertions made"""
    nO, c0, nC = shape
    rows = nO * nC
    monkeypatch.setenv("BIOEM_CONVOLVE_FUSED", "1" if fused else "0")
    conv, params, raw, info = E.debug_convolve_batch(data.proj[:nO], c0, nC, want_raw=True)
    what = (data.N, shape, fused)
    assert info["fused"] == int(fused) and info["rows"] == rows and info["guard"] == 1, (what, info)
    assert conv.shape == (rows + 1, data.N, data.H, 2) and params.shape == (rows + 1,)
    # the guard row and the guard parameters are as the entry filled them; no word of the batch's own rows is
    words, pwords = conv.view(u32).reshape(rows + 1, -1), params.view(u32).reshape(rows + 1, 5)
    assert (words[rows] == 0xFFFFFFFF).all() and (pwords[rows] == 0xFFFFFFFF).all(), what
    for r in range(rows):
        assert not (words[r] == 0xFFFFFFFF).any(), (what, "slot", divmod(r, nC), np.argwhere(words[r] == 0xFFFFFFFF)[:4])
        assert not (pwords[r] == 0xFFFFFFFF).any(), (what, "slot", divmod(r, nC), pwords[r])
    # the bytes as the comparison kernels read them
    assert raw.shape == (rows, data.N * info["Hp"], 2)
    for r in range(rows):
        want, at = cr.comparison_layout(conv[r], info["fast"], info["N1"], info["Hp"])
        assert raw[r][at].tobytes() == want[at].tobytes(), (what, "slot", divmod(r, nC), info)
    return conv[:rows], params[:rows], info


def same_bits(got, want):
    return np.ascontiguousarray(got, dtype=f32).view(u32) == np.ascontiguousarray(want, dtype=f32).view(u32)


def check_ctf_params(params, data, shape, what):
    nO, c0, nC = shape
    for r in range(nO * nC):
        o, c = divmod(r, nC)
        got = [params[r]["amp"], params[r]["pha"], params[r]["env"]]
        assert same_bits(got, data.ctf_param[c0 + c]).all(), (what, "slot", (o, c), got, data.ctf_param[c0 + c])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_kernels"])
@pytest.mark.parametrize("N", cr.SIZES)
def test_class_a_bit_for_bit(N, fused, monkeypatch):
    a = cr.class_a(N)
    E = engine_of(N)
    E.upload_ctf(a.ctf, a.ctf_param)
    ulps = 0
    for shape in cr.shapes_of(N):
        nO, c0, nC = shape
        what = (N, shape, "fused" if fused else "two kernels")
        conv, params, info = run_batch(E, a, shape, fused, monkeypatch)
        check_ctf_params(params, a, shape, what)
        for r in range(nO * nC):
            o, c = divmod(r, nC)
            slot = (what, "slot", (o, c))
            bad = ~same_bits(conv[r], a.conv[o, c0 + c])
            assert not bad.any(), (slot, np.argwhere(bad)[:4], conv[r][bad][:4], a.conv[o, c0 + c][bad][:4])
            assert same_bits(params[r]["sumC"], a.sumC[o, c0 + c]), (slot, params[r]["sumC"], a.sumC[o, c0 + c])
            got, want = f32(params[r]["sumsquareC"]), f32(a.sumsq[o, c0 + c])
            ulps = max(ulps, abs(int(got.view(np.int32)) - int(want.view(np.int32))))
            assert same_bits(got, want), (slot, got, want, "chain", a.chain[o, c0 + c])
    print("N %d %s: sumsquareC off by at most %d ulp" % (N, "fused" if fused else "two kernels", ulps))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_kernels"])
@pytest.mark.parametrize("N", cr.SIZES)
def test_class_b_within_the_rounding_bounds(N, fused, monkeypatch):
    b = cr.class_b(N)
    E = engine_of(N)
    E.upload_ctf(b.ctf, b.ctf_param)
    worst = {"spectrum": 0.0, "sumsquareC": 0.0}
    for shape in cr.shapes_of(N):
        nO, c0, nC = shape
        what = (N, shape, "fused" if fused else "two kernels")
        conv, params, info = run_batch(E, b, shape, fused, monkeypatch)
        check_ctf_params(params, b, shape, what)
        for r in range(nO * nC):
            o, c = divmod(r, nC)
            slot = (what, "slot", (o, c))
            for k, exact, mag in ((0, b.re, b.mag_re), (1, b.im, b.mag_im)):
                err = np.abs(conv[r][..., k].astype(np.float64) - exact[o, c0 + c])
                bound = 2 * U * mag[o, c0 + c]
                bad = ~(err <= bound)                              # (no bin exempt: a zero bound asks for the exact value)
                assert not bad.any(), (slot, k, np.argwhere(bad)[:4], err[bad][:4], bound[bad][:4])
                with np.errstate(all="ignore"):
                    worst["spectrum"] = max(worst["spectrum"], float(np.where(bound > 0, err / bound, 0.0).max()))
            assert same_bits(params[r]["sumC"], conv[r][0, 0, 0]), (slot, params[r]["sumC"], conv[r][0, 0])
            exact = cr.weighted_fsum(conv[r], N) / (N * N)
            err, bound = abs(float(params[r]["sumsquareC"]) - exact), (b.M + 3) * U * exact
            assert err <= bound, (slot, params[r]["sumsquareC"], exact, err / bound)
            worst["sumsquareC"] = max(worst["sumsquareC"], err / bound)
    print("N %d %s: largest achieved fraction of the bound: spectrum %.3f, sumsquareC %.4f"
          % (N, "fused" if fused else "two kernels", worst["spectrum"], worst["sumsquareC"]))


def test_the_sizes_cover_both_layouts_and_a_padded_pitch(monkeypatch):
    a = {N: cr.class_a(N) for N in cr.SIZES}
    infos = {}
    for N in cr.SIZES:
        E = engine_of(N)
        E.upload_ctf(a[N].ctf, a[N].ctf_param)
        infos[N] = run_batch(E, a[N], (1, 0, 1), True, monkeypatch)[2]
    print({N: (i["fast"], i["N1"], i["Hp"]) for N, i in infos.items()})
    assert any(i["fast"] == 0 for i in infos.values()) and any(i["fast"] > 0 for i in infos.values()), infos
    assert any(i["Hp"] > N // 2 + 1 for N, i in infos.items()), infos
    assert all(i["guard"] == 1 for i in infos.values())
    for N, i in infos.items():
        assert i["Hp"] == N // 2 + 1 or i["fast"], (N, i)
        assert not i["fast"] or i["N1"] * 2 * i["fast"] == N, (N, i)


def test_invalid_arguments_are_refused(monkeypatch):
    """2 and a message for each, and the next good call on the same handle is right to the bit"""
    N = 64
    a = cr.class_a(N)
    E = engine_of(N)
    E.upload_ctf(a.ctf, a.ctf_param)
    old = _engines.pop(10, None)                            # a new handle: its CTF sets are not uploaded yet
    if old is not None:
        old.close()
    small = cr.class_a(10)
    with pytest.raises(RuntimeError, match="CTF kernels not uploaded") as ei:
        engine_of(10).debug_convolve_batch(small.proj[:1], 0, 1)
    assert ei.value.rc == 2
    engine_of(10).upload_ctf(small.ctf, small.ctf_param)
    run_batch(engine_of(10), small, (1, 0, 1), True, monkeypatch)

    def good():
        conv, params, _ = run_batch(E, a, (2, 3, 4), True, monkeypatch)
        assert same_bits(conv, a.conv[:2, 3:7].reshape(8, N, a.H, 2)).all()
        assert same_bits(params["sumsquareC"], a.sumsq[:2, 3:7].reshape(-1)).all()

    good()
    more = np.zeros((N_ANGLES + 1, N, a.H, 2), dtype=f32)
    for proj, c0, nC, match in [(a.proj[:0], 0, 1, "orientations per call"), (more, 0, 1, "orientations per call"),
                                (a.proj[:1], -1, 1, "CTF range"), (a.proj[:1], 0, 0, "CTF range"),
                                (a.proj[:1], 1, cr.N_CTF, "CTF range"), (a.proj[:1], cr.N_CTF, 1, "CTF range"),
                                (more[:N_ANGLES], 0, cr.N_CTF, "guard row")]:
        with pytest.raises(RuntimeError, match=match) as ei:
            E.debug_convolve_batch(proj, c0, nC)
        assert ei.value.rc == 2
        good()
    # a null pointer for each required argument
    conv = np.zeros((2, N, a.H, 2), dtype=f32)
    params = np.zeros(2 * 5, dtype=f32)
    info = np.zeros(6, dtype=np.int32)
    spec = np.ascontiguousarray(a.proj[:1])
    ptr = [x.ctypes.data_as(ctypes.c_void_p) for x in (spec, conv, params, info)]
    for k in range(4):
        p = list(ptr)
        p[k] = None
        assert E.L.bioem_hip_debug_convolve_batch(E.h, p[0], 1, 0, 1, p[1], p[2], None, p[3]) == 2
        assert b"null argument" in E.L.bioem_hip_last_error(E.h)
        good()
