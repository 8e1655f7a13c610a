"""GPU test of what the analysis entries say when they refuse (return 2): the whole bioem_hip_last_error string of every reason
of render_best_maps, best_match_rings, debug_ring_sums, view_sums, view_averages, window_posterior, ctf_scan, debug_ctf_scan,
model_gradient and debug_grad_image, and of every "not uploaded" state of the entries that need one.

The expected strings are written out here from the formats of the entries as they were before they came to share their
validation (one snprintf per entry then), filled with the values of the input that is refused; none is taken from the code
under test.  After every refusal the same entry, on good input, returns the bytes it returned before."""
import ctypes as C

import numpy as np
import pytest

from test_best_rings_gpu import random_spectra, scene
from test_model_gradient_gpu import image_inputs

pytestmark = pytest.mark.gpu

OWN = "no per-particle orientation lists (bioem_hip_upload_particle_orientation_lists)"
ENTRIES = ["render_best_maps", "best_match_rings", "debug_ring_sums", "view_sums", "view_averages", "window_posterior",
           "ctf_scan", "debug_ctf_scan", "model_gradient", "debug_grad_image"]


def rc_of(call):
    """the return code of an entry: of the library function itself, or the one the Engine method raises with"""
    try:
        rc = call()
    except RuntimeError as e:
        return e.rc
    return rc if isinstance(rc, int) else 0


def joined(x):
    if isinstance(x, dict):
        x = [x[k] for k in sorted(x)]
    return b"".join(a.tobytes() for a in (x if isinstance(x, (tuple, list)) else [x]))


class Inputs:
    """good input of every entry on the scene of the ring tests at N = 32 with 14 records"""

    def __init__(self):
        import bioem_amd.engine as eng
        sc = self.sc = scene(32)
        n = self.n = sc.nRec
        assert sc.N == 32 and n == 14
        self.rec = sc.records()
        self.g = (np.arange(n) % 3).astype(np.int32)
        self.w = np.ones(n)
        self.orient = np.array([0, sc.nA - 1, 1], dtype=np.int32)
        self.R, self.P = random_spectra(n, 32, 64, 3.0), random_spectra(n, 32, 65, 0.5)
        self.wreq = np.zeros(3, dtype=eng.WINDOW_REQUEST_DTYPE)
        self.sreq = np.zeros(3, dtype=eng.SCAN_REQUEST_DTYPE)
        self.greq = np.zeros(3, dtype=eng.GRAD_REQUEST_DTYPE)
        for i, (p, o, c, x, y) in enumerate([(0, 0, 0, 0, 0), (1, sc.nA - 1, sc.nCTF - 1, 31, -31), (0, 1, 0, -3, 2)]):
            self.wreq[i] = (p, o, c)
            self.sreq[i] = (p, o, x, y)
            self.greq[i] = (p, o, c, x, y)
        self.K, self.par3 = sc.refCTF[:2], sc.ctfParam[:2]
        self.D, self.conv, self.par5 = image_inputs(32, 2)
        self.ref = {e: joined(self.good(e, sc.engine)()) for e in ENTRIES}

    def good(self, entry, E, own=False):
        D = self.D
        return {
            "render_best_maps": lambda: E.render_best_maps(self.rec, own=own),
            "best_match_rings": lambda: E.best_match_rings(self.rec, own=own),
            "debug_ring_sums": lambda: E.debug_ring_sums(self.R, self.P, self.rec),
            "view_sums": lambda: E.view_sums(self.rec, self.g),
            "view_averages": lambda: E.view_averages(self.rec, self.g, self.orient),
            "window_posterior": lambda: E.window_posterior(self.wreq, own=own),
            "ctf_scan": lambda: E.ctf_scan(self.sreq, self.K, self.par3, own=own),
            "debug_ctf_scan": lambda: E.debug_ctf_scan(D["P"][:2], D["F"][:2], D["sumRef"][:2], D["sumsqRef"][:2],
                                                       D["shifts"][:2], D["K"][:2], D["par3"][:2]),
            "model_gradient": lambda: E.model_gradient(self.greq, own=own),
            "debug_grad_image": lambda: E.debug_grad_image(self.conv, D["F"][:2], D["K"][:2], self.par5, D["sumRef"][:2],
                                                           D["sumsqRef"][:2], D["shifts"][:2]),
        }[entry]

    def table(self):
        """(entry, the call that is refused, the handle's whole message)"""
        sc, E, L, n, nA, nC = self.sc, self.sc.engine, self.sc.engine.L, self.n, self.sc.nA, self.sc.nCTF
        rec, g, w, orient, D = self.rec, self.g, self.w, self.orient, self.D
        T = []

        def with_field(a, i, field, value):
            b = a.copy()
            b[i][field] = value
            return b

        def with_item(a, i, value):
            b = a.copy()
            b[i] = value
            return b

        # ---- best-match records ----
        bad_records = [("orient", nA, "max_prob_orient outside its orientation list"),
                       ("orient", -1, "max_prob_orient outside its orientation list"),
                       ("conv", nC, "max_prob_conv outside [0, nCTF)"), ("conv", -1, "max_prob_conv outside [0, nCTF)"),
                       ("cent_x", 32, "displacement of N pixels or more"), ("cent_x", -32, "displacement of N pixels or more"),
                       ("cent_y", 32, "displacement of N pixels or more"), ("cent_y", -32, "displacement of N pixels or more")]
        for entry, fn, lib in (("render_best_maps", E.render_best_maps, L.bioem_hip_render_best_maps),
                               ("best_match_rings", E.best_match_rings, L.bioem_hip_best_match_rings)):
            T.append((entry, lambda lib=lib: lib(E.h, None, 0, 0, n, None), entry + ": null argument"))
            for a in ((5, 2), (4, 4), (0, n + 1), (-1, 3)):
                T.append((entry, lambda fn=fn, a=a: fn(rec, *a),
                          entry + ": particle range empty, reversed or outside [0, nMaps)"))
            T.append((entry, lambda fn=fn: fn(rec, own=True), entry + ": " + OWN))
            for field, value, why in bad_records:
                b = with_field(rec, 3, field, value)
                r = b[3]
                T.append((entry, lambda fn=fn, b=b: fn(b),
                          "%s: particle 3: %s (orient %d of %d, conv %d, cent %d %d)"
                          % (entry, why, r["orient"], nA, r["conv"], r["cent_x"], r["cent_y"])))
        T.append(("debug_ring_sums", lambda: L.bioem_hip_debug_ring_sums(E.h, None, None, None, 1, None),
                  "debug_ring_sums: null argument or no images"))
        T.append(("debug_ring_sums", lambda: E.debug_ring_sums(self.R[:0], self.P[:0], rec[:0]),
                  "debug_ring_sums: null argument or no images"))
        for field, value, _ in bad_records[2:]:
            b = with_field(rec, 5, field, value)
            r = b[5]
            T.append(("debug_ring_sums", lambda b=b: E.debug_ring_sums(self.R, self.P, b),
                      "debug_ring_sums: image 5: max_prob_conv outside [0, nCTF) or a displacement of N pixels or more "
                      "(conv %d, cent %d %d)" % (r["conv"], r["cent_x"], r["cent_y"])))

        # ---- the members of views ----
        T.append(("view_sums", lambda: L.bioem_hip_view_sums(E.h, None, None, None, 3, 0, 3, None, None, None),
                  "view_sums: null argument"))
        T.append(("view_averages", lambda: L.bioem_hip_view_averages(E.h, None, None, None, None, 3, 0.1, 0, 3, None, None, None),
                  "view_averages: null argument"))
        for value in (-0.1, np.nan, np.inf):
            T.append(("view_averages", lambda value=value: E.view_averages(rec, g, orient, wiener=value),
                      "view_averages: wiener negative or not finite"))
        for entry, call in (("view_sums", lambda r_=rec, g_=g, w_=None, **kw: E.view_sums(r_, g_, w_, **kw)),
                            ("view_averages", lambda r_=rec, g_=g, w_=None, **kw: E.view_averages(r_, g_, orient, w_, **kw))):
            for g0, g1 in ((2, 1), (1, 1), (0, 4), (-1, 2)):
                T.append((entry, lambda call=call, g0=g0, g1=g1: call(g0=g0, g1=g1),
                          entry + ": group range empty, reversed or outside [0, nGroups)"))
            r = rec[2]
            for value in (3, -2):
                kw = {"n_groups": 3} if entry == "view_sums" else {}  # (view_averages: as many as it has orientations)
                T.append((entry, lambda call=call, value=value, kw=kw: call(g_=with_item(g, 2, value), **kw),
                          "%s: particle 2: group outside [0, nGroups) and not -1 (group %d of 3, weight 1, conv %d, cent %d %d)"
                          % (entry, value, r["conv"], r["cent_x"], r["cent_y"])))
            r = rec[7]
            for value, text in ((-1.0, "-1"), (-0.25, "-0.25"), (np.inf, "inf"), (np.nan, "nan")):
                T.append((entry, lambda call=call, value=value: call(w_=with_item(w, 7, value)),
                          "%s: particle 7: weight negative or not finite (group %d of 3, weight %s, conv %d, cent %d %d)"
                          % (entry, g[7], text, r["conv"], r["cent_x"], r["cent_y"])))
            for field, value, why in bad_records[2:]:
                b = with_field(rec, 4, field, value)
                r = b[4]
                T.append((entry, lambda call=call, b=b: call(r_=b),
                          "%s: particle 4: %s (group %d of 3, weight 1, conv %d, cent %d %d)"
                          % (entry, why, g[4], r["conv"], r["cent_x"], r["cent_y"])))
        for value in (nA, -2):
            T.append(("view_averages", lambda value=value: E.view_averages(rec, g, with_item(orient, 1, value)),
                      "view_averages: group 1: orientation %d outside the list of %d and not -1" % (value, nA)))

        # ---- requests ----
        def request_rows(entry, call, req, fields, tail):
            T.append((entry, lambda: call(req[:0]), entry + ": null argument or no requests"))
            T.append((entry, lambda: call(req, own=True), entry + ": " + OWN))
            for field, value, why in fields:
                b = with_field(req, 2, field, value)
                r = b[2]
                inside = 0 <= r["particle"] < n
                T.append((entry, lambda b=b: call(b),
                          "%s: request 2: %s (particle %d of %d, orient %d of %d%s)"
                          % (entry, why, r["particle"], n, r["orient"], nA if inside else 0, tail(r))))

        who = [("particle", n, "particle outside [0, nMaps)"), ("particle", -1, "particle outside [0, nMaps)"),
               ("orient", nA, "orient outside its orientation list"), ("orient", -1, "orient outside its orientation list")]
        conv = [("conv", nC, "conv outside [0, nCTF)"), ("conv", -1, "conv outside [0, nCTF)")]
        shift = [(f, v, "shift outside (-N, N)") for f in ("shiftX", "shiftY") for v in (32, -32)]
        request_rows("window_posterior", E.window_posterior, self.wreq, who + conv,
                     lambda r: ", conv %d of %d" % (r["conv"], nC))
        request_rows("ctf_scan", lambda q, **kw: E.ctf_scan(q, self.K, self.par3, **kw), self.sreq, who + shift,
                     lambda r: ", shift %d %d, N 32" % (r["shiftX"], r["shiftY"]))
        request_rows("model_gradient", E.model_gradient, self.greq, who + conv + shift,
                     lambda r: ", conv %d of %d, shift %d %d, N 32" % (r["conv"], nC, r["shiftX"], r["shiftY"]))
        r = self.greq[1]
        for value in (np.nan, np.inf, -np.inf):
            T.append(("model_gradient", lambda value=value: E.model_gradient(self.greq, weights=np.array([1.0, value, 1.0])),
                      "model_gradient: request 1: weight not finite (particle %d of %d, orient %d of %d, conv %d of %d, "
                      "shift %d %d, N 32)" % (r["particle"], n, r["orient"], nA, r["conv"], nC, r["shiftX"], r["shiftY"])))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        coef, logp = np.zeros((3, 4)), np.zeros((3, 2))
        T.append(("model_gradient", lambda: L.bioem_hip_model_gradient(E.h, vp(self.greq), None, 3, 0, None, None, None, vp(coef)),
                  "model_gradient: grad_out and points_out both null"))
        T.append(("window_posterior", lambda: L.bioem_hip_window_posterior(E.h, vp(self.wreq), 3, 0, None, None, None),
                  "window_posterior: null argument or no requests"))
        T.append(("ctf_scan", lambda: E.ctf_scan(self.sreq, self.K[:0], self.par3[:0]), "ctf_scan: no candidates (G = 0)"))
        k, t = np.ascontiguousarray(self.K, dtype=np.float32), np.ascontiguousarray(self.par3, dtype=np.float32)
        T.append(("ctf_scan", lambda: L.bioem_hip_ctf_scan(E.h, vp(self.sreq), 3, 0, vp(k), vp(t), -7, vp(logp), None, None),
                  "ctf_scan: no candidates (G = -7)"))
        T.append(("ctf_scan", lambda: L.bioem_hip_ctf_scan(E.h, vp(self.sreq), 3, 0, None, vp(t), 2, vp(logp), None, None),
                  "ctf_scan: null candidate kernels or parameters"))
        T.append(("ctf_scan", lambda: L.bioem_hip_ctf_scan(E.h, vp(self.sreq), 3, 0, vp(k), None, 2, vp(logp), None, None),
                  "ctf_scan: null candidate kernels or parameters"))

        # ---- the hooks that take shifts ----
        two = (D["P"][:2], D["F"][:2], D["sumRef"][:2], D["sumsqRef"][:2])
        T.append(("debug_ctf_scan", lambda: E.debug_ctf_scan(*two, D["shifts"][:2], D["K"][:0], D["par3"][:0]),
                  "debug_ctf_scan: null argument, no records or no candidates"))
        T.append(("debug_grad_image", lambda: L.bioem_hip_debug_grad_image(E.h, None, None, None, None, None, None, None, 2, None, None),
                  "debug_grad_image: null argument or no records"))
        for axis in (0, 1):
            for value in (32, -32):
                sh = with_field(D["shifts"][:2], 1, axis, value)
                text = "record 1: shift outside (-N, N) (shift %d %d, N 32)" % (sh[1][0], sh[1][1])
                T.append(("debug_ctf_scan", lambda sh=sh: E.debug_ctf_scan(*two, sh, D["K"][:2], D["par3"][:2]),
                          "debug_ctf_scan: " + text))
                T.append(("debug_grad_image", lambda sh=sh: E.debug_grad_image(self.conv, D["F"][:2], D["K"][:2], self.par5,
                                                                                D["sumRef"][:2], D["sumsqRef"][:2], sh),
                          "debug_grad_image: " + text))
        return T


_inputs = []


def inputs():
    if not _inputs:
        _inputs.append(Inputs())
    return _inputs[0]


def check(I, E, entry, call, want, own=False, ref=None):
    assert rc_of(call) == 2, (entry, want)
    got = E.L.bioem_hip_last_error(E.h).decode()
    assert got == want, entry
    assert joined(I.good(entry, E, own)()) == (I.ref[entry] if ref is None else ref), (entry, want)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_reason_word_for_word(entry):
    I = inputs()
    rows = [t for t in I.table() if t[0] == entry]
    assert len({want for _, _, want in rows}) >= 2
    for _, call, want in rows:
        check(I, I.sc.engine, entry, call, want)
    print("%s: %d refusals, %d different messages" % (entry, len(rows), len({want for _, _, want in rows})))


def test_every_entry_of_the_table_is_an_entry_of_the_list():
    I = inputs()
    assert {t[0] for t in I.table()} == set(ENTRIES)


def test_not_uploaded_states_word_for_word():
    """a handle filled step by step, in the order the entries name what is missing: model, CTF kernels, orientations (or own
    lists), particles; view_averages names the CTF kernels first"""
    import bioem_amd.engine as eng
    I = inputs()
    sc = I.sc
    E = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)
    needs_all = ["best_match_rings", "window_posterior", "model_gradient"]
    with_lists = needs_all + ["render_best_maps", "ctf_scan"]
    MODEL, CTF, ORIENT, PARTICLES = ("model not uploaded", "CTF kernels not uploaded", "orientations not uploaded",
                                     "particles not uploaded")
    steps = [  # (the upload, what each entry then names first, what it names when asked for own lists)
        (lambda: None,
         dict({e: MODEL for e in with_lists}, debug_ring_sums=CTF, view_sums=CTF, view_averages=CTF), MODEL),
        (lambda: E.upload_model(sc.points, sc.NormDen, sc.px, *sc.shift),
         dict({e: CTF for e in needs_all}, render_best_maps=CTF, debug_ring_sums=CTF, view_sums=CTF, view_averages=CTF,
              ctf_scan=ORIENT), None),
        (lambda: E.upload_ctf(sc.refCTF, sc.ctfParam),
         dict({e: ORIENT for e in with_lists}, view_averages=ORIENT, view_sums=PARTICLES), OWN),
        (lambda: E.upload_orientations(sc.angles, sc.isQuat),
         dict({e: PARTICLES for e in needs_all}, ctf_scan=PARTICLES, view_averages=PARTICLES, view_sums=PARTICLES), OWN),
    ]
    for step, shared, own in steps:
        step()
        for entry, why in shared.items():
            assert rc_of(I.good(entry, E)) == 2, (entry, why)
            assert E.L.bioem_hip_last_error(E.h).decode() == entry + ": " + why
        for entry in with_lists if own else []:
            assert rc_of(I.good(entry, E, own=True)) == 2, (entry, own)
            assert E.L.bioem_hip_last_error(E.h).decode() == entry + ": " + own
    assert joined(I.good("render_best_maps", E)()) == I.ref["render_best_maps"]  # (needs no particles)
    E.upload_particle_maps(sc.maps)
    for entry in ENTRIES:
        assert joined(I.good(entry, E)()) == I.ref[entry], entry
    E.close()
    # view_averages after the CTF kernels: the model, which the other entries name first
    E = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)
    E.upload_ctf(sc.refCTF, sc.ctfParam)
    assert rc_of(I.good("view_averages", E)) == 2
    assert E.L.bioem_hip_last_error(E.h).decode() == "view_averages: model not uploaded"
    assert joined(I.good("debug_ring_sums", E)()) == I.ref["debug_ring_sums"]
    E.close()


def test_an_index_beyond_an_own_list_names_that_list():
    """own lists of 3, 2, 2, ... orientations: the length in the message is the list's of the particle"""
    I = inputs()
    sc = I.sc
    E = sc.make_engine(sc.nRec)
    E.upload_particle_maps(sc.maps)
    E.upload_particle_orientation_lists([sc.angles[:3]] + [sc.angles[:2]] * (sc.nRec - 1), sc.isQuat)
    rec = I.rec.copy()
    rec["orient"] = 1
    wreq, sreq, greq = I.wreq.copy(), I.sreq.copy(), I.greq.copy()
    for q in (wreq, sreq, greq):
        q["orient"] = 1
    J = Inputs.__new__(Inputs)
    J.__dict__.update(I.__dict__)
    J.rec, J.wreq, J.sreq, J.greq = rec, wreq, sreq, greq
    nC = sc.nCTF

    def bad(a, i, value):
        b = a.copy()
        b[i]["orient"] = value
        return b

    b = bad(rec, 1, 2)
    tail = "(orient 2 of 2, conv %d, cent %d %d)" % (b[1]["conv"], b[1]["cent_x"], b[1]["cent_y"])
    rows = [("render_best_maps", lambda: E.render_best_maps(b, own=True),
             "render_best_maps: particle 1: max_prob_orient outside its orientation list " + tail),
            ("best_match_rings", lambda: E.best_match_rings(b, own=True),
             "best_match_rings: particle 1: max_prob_orient outside its orientation list " + tail),
            ("window_posterior", lambda: E.window_posterior(bad(wreq, 1, 2), own=True),
             "window_posterior: request 1: orient outside its orientation list (particle 1 of 14, orient 2 of 2, conv %d of %d)"
             % (wreq[1]["conv"], nC)),
            ("ctf_scan", lambda: E.ctf_scan(bad(sreq, 0, 3), I.K, I.par3, own=True),
             "ctf_scan: request 0: orient outside its orientation list (particle 0 of 14, orient 3 of 3, shift 0 0, N 32)"),
            ("model_gradient", lambda: E.model_gradient(bad(greq, 1, 2), own=True),
             "model_gradient: request 1: orient outside its orientation list (particle 1 of 14, orient 2 of 2, conv %d of %d, "
             "shift 31 -31, N 32)" % (greq[1]["conv"], nC))]
    for entry, call, want in rows:
        ref = joined(J.good(entry, E, own=True)())
        check(J, E, entry, call, want, own=True, ref=ref)
    E.close()


def test_a_run_entry_raises_with_its_return_code():
    """the run entries raise as the analysis entries do: the message they always had, and the entry's return code as .rc"""
    I = inputs()
    E = I.sc.engine  # (shared orientations only)
    with pytest.raises(RuntimeError) as e:
        E.compare_own_orientations(0, 1)
    assert str(e.value) == ("compare_own_orientations: compare_own_orientations: no per-particle orientation lists "
                            "(bioem_hip_upload_particle_orientations)")
    assert e.value.rc == 2
    assert joined(I.good("render_best_maps", E)()) == I.ref["render_best_maps"]
