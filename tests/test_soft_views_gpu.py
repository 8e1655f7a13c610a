"""GPU tests of the posterior-weighted view sums (Engine.view_sums_soft, Engine.debug_view_sums_soft,
Engine.reconstruct_soft, Engine.soft_members; include/bioem_hip.h): per group the normal equations
num = sum_r K~ (R W_r - b_r N^2 [k = 0]),  den = sum_r s2_r |K~|^2  over members that carry a table of weighted shifts.

Expected values come from tests/soft_view_reference.py (exact integer arithmetic on the very inputs handed to the kernels,
checked on the CPU by test_soft_views_host.py).  Bounds, all derived there, none read off the device:
  exact class    small integers under shifts of a quarter image: every product and sum is exact, so bit for bit
  rounded class  |num - exact| <= (16 + 2 nd + n_g) 2^-53 sum_r |K~| (|R| sum |a| + |b| N^2 [k = 0]) per component,
                 |den - exact| <= (8 + n_g) 2^-53 sum_r s2 |K~|^2
  hard kernels   the same sums from debug_view_sums within the sum of the two kernels' bounds
  chain          reconstruct_soft is debug_reconstruct on the outputs of view_sums_soft, bit for bit
  planted set    a report, no threshold (see test_planted_set_soft_against_hard)"""
import ctypes as C
import os

import numpy as np
import pytest

import soft_view_reference as sr
import view_reference as vr
from test_best_rings_gpu import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pairs(c):
    return np.ascontiguousarray(np.stack([c.real, c.imag], axis=-1), dtype=np.float32)


def hook_engine(sc, batch, kernels, nMaps=1):
    """a handle with `batch` orientations (its batches and chunks hold that many) and the kernels as its CTF sets"""
    import bioem_amd.engine as eng
    E = eng.Engine(sc.pd, nMaps, batch, len(kernels), algo=1, device=0)
    E.upload_ctf(pairs(kernels), np.tile(sc.ctfParam[:1], (len(kernels), 1)))
    assert 1 <= E.max_batch()[0] <= batch
    return E


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("nd", [1, 2, 3, 5])
def test_exact_class_bit_for_bit(nd):
    """groups of 0, 1, 2 batch + 1, 3 and 2 members on a handle with batches of 3; particles in three groups, a particle
    with no member, the list shuffled"""
    N = 32
    sc = scene(N)
    K = sr.integer_kernels(3, N, nd)
    E = hook_engine(sc, 3, K)
    batch = E.max_batch()[0]
    spec, mem, cells, shifts, nG = sr.exact_problem(nd, [0, 1, 2 * batch + 1, 3, 2], 3, 40 + nd)
    assert max(np.bincount(mem["particle"])) >= 3 and len(spec) - 1 not in mem["particle"] and len(spec) > 2 * batch
    num, den, stats = E.debug_view_sums_soft(spec, mem, cells, shifts, n_groups=nG)
    E.close()
    ex = sr.exact_sums(spec, K, mem, cells, shifts, nG)
    assert not ex[1].any() and not ex[3].any()
    assert num.tobytes() == ex[0].tobytes() and den.tobytes() == ex[2].tobytes()
    assert stats.tobytes() == ex[4].tobytes() and stats[:, 0].tolist() == [0, 1, 2 * batch + 1, 3, 2]
    assert not num[0].any() and not den[0].any() and num[2].any()


@pytest.mark.parametrize("N,nd", [(32, 1), (32, 2), (35, 3), (37, 21), (32, 32), (35, 35), (37, 37)])
def test_rounded_class_against_the_exact_reference(N, nd):
    sc = scene(N)
    K = sr.random_complex(4, N, 5 * N + nd, 1.5)
    spec, mem, cells, shifts, nG = sr.rounded_problem(N, nd, 4, 100 * N + nd)
    assert abs(shifts).max() == N - 1 and (nd < 4 or len(set(shifts.tolist())) < nd)
    E = hook_engine(sc, 3, K)
    num, den, stats = E.debug_view_sums_soft(spec, mem, cells, shifts, n_groups=nG)
    E.close()
    ex = sr.exact_sums(spec, K, mem, cells, shifts, nG)
    an, ad, size = sr.scales(spec, K, mem, cells, nG)
    bn, bd = sr.bounds(an, ad, size, nd)
    en, ed = sr.errors(num, den, ex)
    rn, rd = sr.ratios(en, bn), sr.ratios(ed, bd)
    print("rounded N=%d nd=%d: worst |num - exact| / bound = %.3g, |den - exact| / bound = %.3g" % (N, nd, rn.max(), rd.max()))
    assert (rn <= 1.0).all(), (int(rn.argmax()), rn.max())
    assert (rd <= 1.0).all(), (int(rd.argmax()), rd.max())
    assert np.array_equal(stats[:, 0], size) and not num[2].any() and not den[2].any()
    assert (np.abs(stats[:, 1] - ex[4][:, 1]) <= size * sr.U * ex[4][:, 1]).all()


@pytest.mark.parametrize("N", [32, 37])
def test_against_the_hard_kernels(N):
    """one-hot members against debug_view_sums on the records they stand for, and full 3 x 3 tables against debug_view_sums
    on the ninefold duplicated spectra (norm = a, weight 1, the cell's mu; a and mu multiples of 1 / 8, so b and s2 are
    exact): each within the sum of the two kernels' bounds about the exact value"""
    import bioem_amd.engine as eng
    sc = scene(N)
    E = sc.engine
    rng = np.random.default_rng(N)
    n = 9
    spec = sr.random_complex(n, N, N + 1, 3.0)
    shifts = np.array([-(N - 1), 0, 5], dtype=np.int32)
    nd = len(shifts)
    rec = np.zeros(n, dtype=eng.PROB_MAP_DTYPE)
    rec["cent_x"], rec["cent_y"] = shifts[rng.integers(0, nd, n)], shifts[rng.integers(0, nd, n)]
    rec["conv"] = np.arange(n) % sc.nCTF
    rec["norm"], rec["mu"] = rng.integers(-8, 9, n) * 0.25, rng.integers(-8, 9, n) * 0.5
    w = rng.integers(1, 5, n) * 0.5
    g = np.array([0, 1, 0, 2, 0, 1, 0, 0, -1], dtype=np.int32)
    mem = np.zeros(n, dtype=sr.MEMBER_DTYPE)
    cells = np.zeros((n, nd, nd))
    for p in range(n):
        a = w[p] * float(rec[p]["norm"])
        cells[p, shifts.tolist().index(rec[p]["cent_x"]), shifts.tolist().index(rec[p]["cent_y"])] = a
        mem[p] = (p, g[p], rec[p]["conv"], 0, a * float(rec[p]["norm"]), a * float(rec[p]["mu"]), w[p])
    hard = E.debug_view_sums(spec, rec, g, w, n_groups=3)
    soft = E.debug_view_sums_soft(spec, mem, cells, shifts, n_groups=3)
    bh = vr.bounds(*vr.scales(spec, sc.refCTF, rec, w, g, 3))
    an, ad, size = sr.scales(spec, sc.refCTF, mem, cells, 3)
    bs = sr.bounds(an, ad, size, nd)
    dn = np.maximum(np.abs((soft[0] - hard[0]).real), np.abs((soft[0] - hard[0]).imag))
    rn, rd = sr.ratios(dn, bh[0] + bs[0]), sr.ratios(np.abs(soft[1] - hard[1]), bh[1] + bs[1])
    print("one-hot N=%d: worst |soft - hard| / (bound + bound): num %.3g, den %.3g" % (N, rn.max(), rd.max()))
    assert (rn <= 1.0).all() and (rd <= 1.0).all() and np.array_equal(soft[2], hard[2])
    # full tables
    m2 = mem[:4].copy()
    m2["group"] = [0, 1, 0, 0]
    c2 = rng.integers(-8, 9, (4, nd, nd)) * 0.125
    mus = rng.integers(-8, 9, (4, nd, nd)) * 0.125
    m2["s2"], m2["b"] = (c2 * c2).sum(axis=(1, 2)), (c2 * mus).sum(axis=(1, 2))
    S, r9, g9 = sr.brute_force(spec, m2, c2, mus, shifts)
    rec9 = np.zeros(len(r9), dtype=eng.PROB_MAP_DTYPE)
    for k in r9.dtype.names:
        rec9[k] = r9[k]
    hard = E.debug_view_sums(S.astype(np.complex64), rec9, g9, None, n_groups=2)
    soft = E.debug_view_sums_soft(spec, m2, c2, shifts, n_groups=2)
    bh = vr.bounds(*vr.scales(S, sc.refCTF, rec9, None, g9, 2))
    an, ad, size = sr.scales(spec, sc.refCTF, m2, c2, 2)
    bs = sr.bounds(an, ad, size, nd)
    dn = np.maximum(np.abs((soft[0] - hard[0]).real), np.abs((soft[0] - hard[0]).imag))
    rn, rd = sr.ratios(dn, bh[0] + bs[0]), sr.ratios(np.abs(soft[1] - hard[1]), bh[1] + bs[1])
    print("tables N=%d: worst |soft - hard| / (bound + bound): num %.3g, den %.3g" % (N, rn.max(), rd.max()))
    assert (rn <= 1.0).all() and (rd <= 1.0).all() and soft[0].any()


def scene_members(sc, seed, nd=3):
    """members over the scene's particles: group 2 holds more members than any batch, particle 1 sits in three groups and
    twice in group 2, particles 4 and 11 have no member, one member is left out"""
    n = sc.nRec
    rng = np.random.default_rng(seed)
    plan = [(p, 2, p % sc.nCTF) for p in range(n) if p not in (4, 11)]
    plan += [(1, 0, 1), (1, 1, 0), (1, 2, (1 + sc.nCTF // 2) % sc.nCTF), (0, 0, 0), (5, 1, 2 % sc.nCTF), (6, -1, 0), (9, 0, 1 % sc.nCTF)]
    order = rng.permutation(len(plan))
    mem = np.zeros(len(plan), dtype=sr.MEMBER_DTYPE)
    for r, k in enumerate(order):
        mem[r]["particle"], mem[r]["group"], mem[r]["conv"] = plan[k]
    mem["s2"], mem["b"], mem["mass"] = rng.random(len(plan)) + 0.1, rng.standard_normal(len(plan)), rng.random(len(plan))
    cells = rng.standard_normal((len(plan), nd, nd))
    shifts = np.array([-(sc.N - 1), 2, 2, 0, sc.N - 1][:nd], dtype=np.int32)
    return mem, cells, shifts


@pytest.mark.parametrize("N", [32, 37])
def test_bits_do_not_depend_on_the_call(N):
    """a rerun; sub-ranges; other groups added and removed; the list permuted among different particles; batches of 1, 3
    and 64; the handle's own particles through k_unreorder against the hook fed with debug_particles"""
    sc = scene(N)
    E = sc.engine
    mem, cells, shifts = scene_members(sc, N)
    OB = E.max_batch()[0]
    assert (mem["group"] == 2).sum() > OB
    ref = E.view_sums_soft(mem, cells, shifts)
    assert ref[0].shape == (3, N, N // 2 + 1) and ref[2][:, 0].tolist() == [3, 2, sc.nRec - 2 + 1]
    assert same(ref, E.view_sums_soft(mem, cells, shifts))
    for k in range(3):
        one = E.view_sums_soft(mem, cells, shifts, k, k + 1)
        assert all(x[0].tobytes() == y[k].tobytes() for x, y in zip(one, ref)), k
    sub = E.view_sums_soft(mem, cells, shifts, 1, 3)
    assert all(x.tobytes() == y[1:].tobytes() for x, y in zip(sub, ref))
    # group 2 alone under another label; the other groups split further
    alone = mem.copy()
    alone["group"] = np.where(mem["group"] == 2, 0, -1)
    a = E.view_sums_soft(alone, cells, shifts)
    assert all(x[0].tobytes() == y[2].tobytes() for x, y in zip(a, ref))
    more = mem.copy()
    more["group"] = np.where(mem["group"] == 2, 5, np.where(mem["group"] >= 0, np.arange(len(mem)) % 4, -1))
    b = E.view_sums_soft(more, cells, shifts, n_groups=7)
    assert all(x[5].tobytes() == y[2].tobytes() for x, y in zip(b, ref)) and not b[0][6].any()
    # the list permuted with the members of each particle kept in their order
    perm = np.random.default_rng(1).permutation(len(mem))
    rank = np.empty(len(mem), dtype=np.int64)
    for p in np.unique(mem["particle"]):
        at = np.flatnonzero(mem["particle"][perm] == p)
        rank[at] = np.sort(perm[at])
    assert not np.array_equal(rank, np.arange(len(mem)))
    assert same(ref, E.view_sums_soft(mem[rank], cells[rank], shifts))
    # the hook fed with the spectra the handle holds, on this handle and on handles with batches of 1, 3 and 64
    spectra = E.debug_particles()[0]
    assert same(ref, E.debug_view_sums_soft(spectra, mem, cells, shifts))
    seen = {OB}
    for batch in (1, 3, 64):
        X = hook_engine(sc, batch, vr.as_complex(sc.refCTF), nMaps=sc.nRec)
        seen.add(X.max_batch()[0])
        assert same(ref, X.debug_view_sums_soft(spectra, mem, cells, shifts)), batch
        X.upload_particle_maps(sc.maps)
        assert same(ref, X.view_sums_soft(mem, cells, shifts)), batch
        X.close()
    assert len(seen) >= 3 and min(seen) == 1   # one particle per batch, a few, many


def test_every_handle_kind_gives_the_same_bytes(monkeypatch):
    import bioem_amd.engine as eng
    sc = scene(32)
    mem, cells, shifts = scene_members(sc, 7)
    ref = sc.engine.view_sums_soft(mem, cells, shifts)
    for kw in (dict(algo=2), dict(shard=(2, 4))):
        X = sc.make_engine(sc.nRec, **kw)
        X.upload_particle_maps(sc.maps)
        assert same(ref, X.view_sums_soft(mem, cells, shifts)), kw
        X.close()
    with monkeypatch.context() as m:
        m.setenv("BIOEM_CC_DIRECT", "1")
        X = sc.make_engine(sc.nRec)
        assert X.kernel_signature.startswith("k_compare_direct")
        X.upload_particle_maps(sc.maps)
        assert same(ref, X.view_sums_soft(mem, cells, shifts))
        X.close()
    X = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)   # no model, no orientations
    X.upload_ctf(sc.refCTF, sc.ctfParam)
    X.upload_particle_maps(sc.maps)
    assert same(ref, X.view_sums_soft(mem, cells, shifts))
    X.close()


def chain_matches(E, sc, mem, cells, shifts, orient, angles=None):
    """reconstruct_soft against debug_reconstruct fed the outputs of view_sums_soft: bit for bit"""
    got = E.reconstruct_soft(mem, cells, orient, shifts, want_spec=True)
    num, den, stats = E.view_sums_soft(mem, cells, shifts, n_groups=len(orient))
    used = [v for v in range(len(orient)) if orient[v] >= 0 and stats[v, 0] > 0]
    ang = (sc.angles if angles is None else angles)[np.asarray(orient)[used]]
    want = E.debug_reconstruct(num[used], den[used], ang, isQuat=sc.isQuat)
    assert got["vol"].tobytes() == want["vol"].tobytes() and got["spec"].tobytes() == want["spec"].tobytes()
    assert got["den"].tobytes() == want["denV"].tobytes() and np.abs(got["vol"]).max() > 0
    inside = np.isin(mem["group"], used)
    order = np.lexsort((np.arange(len(mem)), mem["particle"]))
    mass = 0.0
    for r in order:
        if inside[r]:
            mass += mem["mass"][r]
    assert got["stats"][:3].tolist() == [float(len(used)), float(inside.sum()), mass]
    return got, used


def test_chain_on_hand_made_members():
    sc = scene(32)
    E = sc.engine
    mem, cells, shifts = scene_members(sc, 3)
    orient = np.array([sc.nA - 1, -1, 0, 1], dtype=np.int32)   # group 1 without an orientation, group 3 without members
    got, used = chain_matches(E, sc, mem, cells, shifts, orient)
    assert used == [0, 2]
    again = E.reconstruct_soft(mem, cells, orient, shifts, want_spec=True)
    assert all(got[k].tobytes() == again[k].tobytes() for k in ("vol", "spec", "den", "stats"))
    X = sc.make_engine(sc.nRec, shard=(0, 1))   # chunks of one view, batches of one particle
    X.upload_particle_maps(sc.maps)
    assert X.max_batch()[0] == 1
    other = X.reconstruct_soft(mem, cells, orient, shifts, want_spec=True)
    X.close()
    assert all(got[k].tobytes() == other[k].tobytes() for k in ("vol", "spec", "den", "stats"))


def run_with_table(sc, K):
    """a shard handle over every orientation (its angle table stays on the device) after a real run on the scene's
    particles: (engine, the run's records, the K best orientations per particle)"""
    import bioem_amd.engine as eng
    import oracle as orc
    pd = eng.ParamDevice()
    for f, _ in eng.ParamDevice._fields_:
        setattr(pd, f, getattr(sc.pd, f))
    pd.writeAngles = K
    E = eng.Engine(pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0, shard=(0, sc.nA))
    E.upload_ctf(sc.refCTF, sc.ctfParam)
    E.upload_model(sc.points, sc.NormDen, sc.px, *sc.shift)
    E.upload_orientations(sc.angles, sc.isQuat)
    E.upload_particle_maps(sc.maps)
    raw, pmap, _ = eng.new_prob_block(sc.nRec, 0, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, sc.nA)
    E.finish_run(raw)
    return E, pmap, E.topk_angles(K, orc.logp_constant(pd))


def test_chain_after_a_real_run():
    """soft_members(K = 1) and (K = 3, from topk_angles) after a run on scene(32): the masses of a particle add up to 1,
    the chain is the kernels on the view sums, and the half-set weights keep the even and the odd particles"""
    from bioem_amd import reconstruct as rc
    sc = scene(32)
    K = min(3, sc.nA)
    E, pmap, cand = run_with_table(sc, K)
    orient = np.arange(sc.nA, dtype=np.int32)
    for k in (1, K):
        mem, cells, req = E.soft_members(pmap, K=k, topk=cand)
        assert len(mem) == sc.nRec * k * sc.nCTF and np.array_equal(mem["group"], req["orient"])
        per = np.bincount(mem["particle"], weights=mem["mass"], minlength=sc.nRec)
        assert (np.abs(per - 1.0) <= 1e-12).all()
        if k == 1:
            assert np.array_equal(req["orient"], np.repeat(pmap["orient"], sc.nCTF))
        else:
            assert np.array_equal(req["orient"][::sc.nCTF].reshape(sc.nRec, k), cand["orient"][:, :k])
        got, used = chain_matches(E, sc, mem, cells, E.window_shifts(), orient)
        assert used == sorted(set(mem["group"].tolist()))
        e, _ = rc.half_weights(sc.nRec)
        half, _, _ = E.soft_members(pmap, K=k, topk=cand, weights=e)
        assert np.array_equal(half["mass"], np.where(mem["particle"] % 2 == 0, mem["mass"], 0.0))
        assert E.reconstruct_soft(half, cells * e[mem["particle"]][:, None, None], orient, want_vol=False)["stats"][1] == len(mem)
    E.close()


def test_planted_set_soft_against_hard():
    """Noise-free particles rendered from planted records, then a real run: the posterior of every particle sits on one
    cell of one CTF set, the cell of the run's own record, so the soft volume (K = 1) is the hard one of the run's records
    up to what distinguishes the members: the hard sums take the record's norm and mu, which the fold evaluates in float,
    the soft ones cell_params, the same expression in double -- a relative difference of the order 2^-24, amplified by the
    cancellation in the expression, that no accumulation bound (2^-53) covers.  A bound of the volumes' difference in terms
    of the two accumulation bounds, carried through the estimate, is therefore out of reach; the correlation and the
    largest difference are reported without a threshold.  Asserted is what the construction guarantees: the largest
    weight of every particle is at the cell and CTF set of its record and holds the particle's mass.  (The planted norm
    and mu are not what the run finds: the fold's expression is the reference's, with its sums over the half spectrum,
    and differs from the planted values by per cent; the hard volume of the planted records is reported beside.)"""
    import bioem_amd.engine as eng
    N = 32
    sc = scene(N)
    rng = np.random.default_rng(5)
    nP = 24
    E = sc.make_engine(nP)
    X = E.window_shifts()
    rec = np.zeros(nP, dtype=eng.PROB_MAP_DTYPE)
    rec["orient"] = np.arange(nP) % sc.nA
    rec["conv"] = (np.arange(nP) // 2) % sc.nCTF
    rec["cent_x"], rec["cent_y"] = rng.choice(X, nP), rng.choice(X, nP)
    rec["norm"], rec["mu"] = 0.5 + rng.random(nP), rng.standard_normal(nP) * 0.1
    E.upload_particle_maps(E.render_best_maps(rec))
    raw, pmap, _ = eng.new_prob_block(nP, sc.nA, 0)
    E.start_run(raw)
    E.project_convolve_compare(0, sc.nA)
    E.finish_run(raw)
    mem, cells, req, w = E.soft_members(pmap, K=1, want_weights=True)
    flat = w.reshape(nP, -1)
    top, at = flat.max(axis=1), flat.argmax(axis=1)
    ix, iy = np.unravel_index(at % (len(X) ** 2), (len(X), len(X)))
    assert np.array_equal(at // (len(X) ** 2), pmap["conv"]) and np.array_equal(X[ix], pmap["cent_x"]) and np.array_equal(X[iy], pmap["cent_y"])
    assert np.array_equal(pmap["conv"], rec["conv"]) and np.array_equal(pmap["cent_x"], rec["cent_x"]) and np.array_equal(pmap["cent_y"], rec["cent_y"])
    assert (top > 0.5).all()
    orient = np.arange(sc.nA, dtype=np.int32)
    soft = E.reconstruct_soft(mem, cells, orient)["vol"].astype(np.float64)
    hard = E.reconstruct(pmap, pmap["orient"].astype(np.int32), orient)["vol"].astype(np.float64)
    planted = E.reconstruct(rec, pmap["orient"].astype(np.int32), orient)["vol"].astype(np.float64)
    a, b = soft - soft.mean(), hard - hard.mean()
    print("planted N=%d, %d particles: smallest arg-max mass %.17g; soft against the hard volume of the run's records: "
          "correlation %.15f, max |soft - hard| = %.3g of max |hard| = %.3g; of the planted records: max |soft - planted| = %.3g; "
          "worst |norm found / norm planted - 1| = %.3g (reported, no threshold)"
          % (N, nP, top.min(), (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()), np.abs(soft - hard).max(),
             np.abs(hard).max(), np.abs(soft - planted).max(), np.abs(pmap["norm"] / rec["norm"] - 1).max()))
    assert np.isfinite(soft).all() and np.abs(soft).max() > 0
    E.close()


def test_refusals_leave_the_handle_usable():
    import bioem_amd.engine as eng
    sc = scene(32)
    E = sc.engine
    N = sc.N
    mem, cells, shifts = scene_members(sc, 9)
    orient = np.array([0, 1, sc.nA - 1], dtype=np.int32)
    ref = E.view_sums_soft(mem, cells, shifts)
    chain = E.reconstruct_soft(mem, cells, orient, shifts, want_spec=True)

    def changed(field, r, value):
        bad = mem.copy()
        bad[r][field] = value
        return bad

    r, r2 = (int(x) for x in np.flatnonzero(mem["group"] >= 0)[[3, 5]])

    def cell(value):
        bad = cells.copy()
        bad[r2, 1, 2] = value
        return bad
    long_shifts = np.zeros(N + 1, dtype=np.int32)
    cases = [
        (lambda: E.view_sums_soft(mem[:0], cells[:0], shifts, n_groups=3), "null argument or no members"),
        (lambda: E.view_sums_soft(mem, np.zeros((len(mem), 0, 0)), shifts[:0]), "nd 0 outside"),
        (lambda: E.view_sums_soft(mem, np.zeros((len(mem), N + 1, N + 1)), long_shifts), "nd %d outside" % (N + 1)),
        (lambda: E.view_sums_soft(mem, cells, np.array([0, N, 1])), "shift 1: %d outside" % N),
        (lambda: E.view_sums_soft(mem, cells, np.array([0, 1, -N])), "shift 2: -%d outside" % N),
        (lambda: E.view_sums_soft(mem, cells, shifts, 2, 2), "group range empty"),
        (lambda: E.view_sums_soft(mem, cells, shifts, 2, 1), "group range empty"),
        (lambda: E.view_sums_soft(mem, cells, shifts, 0, 4), "group range empty"),
        (lambda: E.view_sums_soft(changed("group", r, 3), cells, shifts, n_groups=3), "member %d: group outside" % r),
        (lambda: E.view_sums_soft(changed("group", r, -2), cells, shifts, n_groups=3), "member %d: group outside" % r),
        (lambda: E.view_sums_soft(changed("particle", r, sc.nRec), cells, shifts), "member %d: particle out of range" % r),
        (lambda: E.view_sums_soft(changed("particle", r, -1), cells, shifts), "member %d: particle out of range" % r),
        (lambda: E.view_sums_soft(changed("conv", r, sc.nCTF), cells, shifts), "member %d: conv outside" % r),
        (lambda: E.view_sums_soft(changed("conv", r, -1), cells, shifts), "member %d: conv outside" % r),
        (lambda: E.view_sums_soft(changed("s2", r, np.inf), cells, shifts), "member %d: s2, b or mass not finite" % r),
        (lambda: E.view_sums_soft(changed("b", r, np.nan), cells, shifts), "member %d: s2, b or mass not finite" % r),
        (lambda: E.view_sums_soft(changed("mass", r, -np.inf), cells, shifts), "member %d: s2, b or mass not finite" % r),
        (lambda: E.view_sums_soft(changed("s2", r, -1e-300), cells, shifts), "member %d: s2 or mass negative" % r),
        (lambda: E.view_sums_soft(changed("mass", r, -0.5), cells, shifts), "member %d: s2 or mass negative" % r),
        (lambda: E.view_sums_soft(mem, cell(np.nan), shifts), "member %d: a cell of the table not finite" % r2),
        (lambda: E.view_sums_soft(mem, cell(np.inf), shifts), "member %d: a cell of the table not finite" % r2),
        (lambda: E.debug_view_sums_soft(E.debug_particles()[0][:3], mem, cells, shifts), "particle out of range"),
        (lambda: E.reconstruct_soft(mem, cells, orient, shifts, wiener=float("nan")), "wiener negative or not finite"),
        (lambda: E.reconstruct_soft(mem, cells, orient, shifts, wiener=-1.0), "wiener negative or not finite"),
        (lambda: E.reconstruct_soft(mem, cells, np.array([0, sc.nA, 1]), shifts), "group 1: orientation %d outside" % sc.nA),
        (lambda: E.reconstruct_soft(mem, cells, np.array([0, -2, 1]), shifts), "group 1: orientation -2 outside"),
        (lambda: E.reconstruct_soft(mem, cells, orient[:2], shifts), "group outside"),
        (lambda: E.reconstruct_soft(changed("b", r, np.inf), cells, orient, shifts), "member %d: s2, b or mass not finite" % r),
    ]
    for call, text in cases:
        with pytest.raises(RuntimeError, match=text) as ei:
            call()
        assert ei.value.rc == 2, text
        assert same(ref, E.view_sums_soft(mem, cells, shifts)), text
    # a member that is left out is not read
    out = changed("conv", int(np.flatnonzero(mem["group"] == -1)[0]), 99)
    assert same(ref, E.view_sums_soft(out, cells, shifts))
    # what the wrappers cannot express: a null argument, every output null, unknown flag bits
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    num, den, st = (np.zeros_like(x) for x in ref)
    st4 = np.zeros(4)
    args = [p(mem), p(cells), len(mem), p(shifts), len(shifts)]
    for k in (0, 1, 3):
        a = list(args)
        a[k] = None
        assert E.L.bioem_hip_view_sums_soft(E.h, *a, 3, 0, 3, p(num), p(den), p(st)) == 2
        assert b"view_sums_soft: null argument" in E.L.bioem_hip_last_error(E.h)
    assert E.L.bioem_hip_view_sums_soft(E.h, *args, 3, 0, 3, p(num), None, p(st)) == 2
    assert E.L.bioem_hip_reconstruct_soft(E.h, *args, p(orient), 3, 0.1, 0, None, None, None, None) == 2
    assert b"reconstruct_soft: every output is null" in E.L.bioem_hip_last_error(E.h)
    assert E.L.bioem_hip_reconstruct_soft(E.h, *args, p(orient), 3, 0.1, 4, None, None, None, p(st4)) == 2
    assert b"unknown flag bits" in E.L.bioem_hip_last_error(E.h)
    assert E.L.bioem_hip_reconstruct_soft(E.h, *args, None, 3, 0.1, 0, None, None, None, p(st4)) == 2
    assert same(ref, E.view_sums_soft(mem, cells, shifts))
    again = E.reconstruct_soft(mem, cells, orient, shifts, want_spec=True)
    assert all(chain[k].tobytes() == again[k].tobytes() for k in ("vol", "spec", "den", "stats"))
    # handles that lack what an entry needs
    X = eng.Engine(sc.pd, sc.nRec, sc.nA, sc.nCTF, algo=1, device=0)
    with pytest.raises(RuntimeError, match="CTF kernels not uploaded"):
        X.view_sums_soft(mem, cells, shifts)
    with pytest.raises(RuntimeError, match="CTF kernels not uploaded"):
        X.debug_view_sums_soft(E.debug_particles()[0], mem, cells, shifts)
    X.upload_ctf(sc.refCTF, sc.ctfParam)
    with pytest.raises(RuntimeError, match="particles not uploaded") as ei:
        X.view_sums_soft(mem, cells, shifts)
    assert ei.value.rc == 2
    with pytest.raises(RuntimeError, match="orientations not uploaded"):
        X.reconstruct_soft(mem, cells, orient, shifts)
    X.upload_orientations(sc.angles, sc.isQuat)
    with pytest.raises(RuntimeError, match="particles not uploaded"):
        X.reconstruct_soft(mem, cells, orient, shifts)
    X.upload_particle_maps(sc.maps)
    assert same(ref, X.view_sums_soft(mem, cells, shifts))
    X.close()


def test_phase_records_of_the_three_kernels():
    sc = scene(32)
    E = sc.engine
    mem, cells, shifts = scene_members(sc, 2)
    E.set_phase_timing(True)
    E.view_sums_soft(mem, cells, shifts)
    ph = E.phase_records()
    E.set_phase_timing(False)
    count = [int((ph["phase"] == k).sum()) for k in range(3)]
    assert sorted(set(ph["phase"].tolist())) == [0, 1, 2] and count[0] == count[1] == count[2] >= 2
    assert (ph["iConvEnd"] == len(shifts)).all() and (ph["iConvBegin"] == 0).all()
    assert (ph["seconds"] > 0).all() and ph["iOrientBegin"].min() == 0 and ph["iOrientEnd"].max() == sc.nRec


def test_cli_reconstruct_soft(tmp_path):
    """--Reconstruct FILE --ReconstructSoft 1, and 2 with WRITE_PROB_ANGLES 2, on a golden case: Output_Probabilities,
    ANG_PROB and the hard-assignment volumes are byte for byte those of the run without the option, the text file begins
    with the hard one's text; the soft files exist and parse; for K = 1 the volume is that of Engine.soft_members and
    Engine.reconstruct_soft on the same run up to the order in which host and numpy add a particle's weights (1e-5 of the
    largest voxel, the volumes are float); FILE_soft.mrc read back with --ReadModelMRC starts a run"""
    import bioem_amd.engine as eng
    from bioem_amd import hostlib, reconstruct as rc, soft_views as sv
    from golden_util import load_case, write_case_inputs
    from test_best_maps_gpu import run_cli
    case = load_case("g10_n64")
    d = tmp_path
    text = open(os.path.join(case["dir"], "param.txt")).read()
    assert "WRITE_PROB_ANGLES" not in text and "PRIOR_ANGLES" not in text
    (d / "param2.txt").write_text(text.rstrip("\n") + "\nWRITE_PROB_ANGLES 2\n")
    files = write_case_inputs(case, d)
    inputs = ["--Inputfile", "param2.txt"] + files
    run_cli(inputs + ["--OutputFile", "plain.txt", "--Reconstruct", "hard"], d, BIOEM_ALGO="1")
    ang = open(d / "ANG_PROB", "rb").read()
    S, angles, ref_ctf, par = hostlib.setup_from_files(str(d / "param2.txt"), str(d / "orient.txt") if case["orient_lines"] else None)
    N, nCTF = S.pd.NumberPixels, S.nCTF
    hard_shells, _ = rc.parse(str(d / "hard"))
    vols = {}
    for K in (1, 2):
        name = "recon%d" % K
        out = run_cli(inputs + ["--OutputFile", "out.txt", "--Reconstruct", name, "--ReconstructSoft", str(K)], d, BIOEM_ALGO="1")
        assert name + "_soft_half2.mrc" in out
        assert open(d / "out.txt", "rb").read() == open(d / "plain.txt", "rb").read() and open(d / "ANG_PROB", "rb").read() == ang
        for suffix in (".mrc", "_half1.mrc", "_half2.mrc"):
            assert open(d / (name + suffix), "rb").read() == open(d / ("hard" + suffix), "rb").read(), suffix
            assert os.path.getsize(d / (name + "_soft" + suffix)) == 1024 + 4 * N ** 3
        assert open(d / name).read().startswith(open(d / "hard").read())
        summary, shells = sv.parse(str(d / name))
        nMaps = len(summary)
        assert nMaps == len(case["maps"]) and (summary["requests"] == K * nCTF).all()
        assert (summary["n_eff"] >= 1.0).all() and (summary["mass_argmax"] > 0).all() and (summary["mass_argmax"] <= 1.0).all()
        assert (summary["n_eff"] <= 1.0 / summary["mass_argmax"] ** 2 * (1 + 1e-12)).all()
        assert np.array_equal(shells["weight"], hard_shells["weight"]) and (np.abs(shells["FSC"]) <= 1 + 1e-12).all()
        assert len(rc.parse(str(d / name))[0]) == len(hard_shells)
        vols[K] = rc.read_mrc(str(d / (name + "_soft.mrc")))
        assert np.isfinite(vols[K]).all() and np.abs(vols[K]).max() > 0
    assert not np.array_equal(vols[1], vols[2])
    # K = 1 against the engine's own path on the same inputs
    pts, nden = hostlib.read_model(str(d / "model.txt"), nocentermass=bool(S.nocentermass), pixelSize=S.pixelSize)
    maps = hostlib.read_particles(str(d / "particles.txt"), N)
    E = eng.Engine(S.pd, len(maps), S.nAngles, nCTF, algo=1, device=0)
    E.upload_particle_maps(maps)
    E.upload_ctf(ref_ctf, par)
    E.upload_model(pts, nden, S.pixelSize, S.shiftX, S.shiftY)
    E.upload_orientations(angles, S.isQuat)
    raw, pmap, _ = eng.new_prob_block(len(maps), S.nAngles, S.pd.writeAngles)
    E.start_run(raw)
    E.project_convolve_compare(0, S.nAngles)
    E.finish_run(raw)
    mem, cells, req, w = E.soft_members(pmap, K=1, want_weights=True)
    want = E.reconstruct_soft(mem, cells, np.arange(S.nAngles, dtype=np.int32), wiener=0.1)["vol"]
    E.close()
    dv = np.abs(vols[1].astype(np.float64) - want).max() / np.abs(want).max()
    print("cli K=1: max |volume - engine's| = %.3g of the largest voxel" % dv)
    assert dv <= 1e-5
    ps, one = sv.particle_summary(req, w, len(maps)), sv.parse(str(d / "recon1"))[0]
    assert np.array_equal(ps["requests"], one["requests"]) and np.allclose(ps["n_eff"], one["n_eff"], rtol=1e-9)
    assert np.allclose(ps["mass_argmax"], one["mass_argmax"], rtol=1e-9)
    out = run_cli(["--Inputfile", "param2.txt", "--Modelfile", "recon1_soft.mrc", "--ReadModelMRC", "--Particlesfile",
                   "particles.txt", "--OutputFile", "back.txt"] + (["--ReadOrientation", "orient.txt"] if case["orient_lines"] else []),
                  d, BIOEM_ALGO="1", BIOEM_DEBUG_NMAPS="1", BIOEM_DEBUG_BREAK="2")
    assert "Protein structure read from MRC" in out and os.path.getsize(d / "back.txt") > 0
