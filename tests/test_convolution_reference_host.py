"""The reference of tests/convolution_reference.py against the CPU oracle's orc.convolve (oracle/bioem_oracle.c, built
without contraction), and the conditions the class-A sets of tests/test_convolution_exact_gpu.py have to meet; no device.

A class-A case is one image size with one launch shape (nO, c0, nC): the slots (o, c0 + c) of that launch.  For each case
and each of five wrong summation orders at least one slot's sumsquareC differs in bits from the reference's, so a kernel
that summed in that order fails every launch shape of every size (a single slot coincides with a wrong order in roughly
1 / sqrt(M) of the sets, the rounding walks of two orders ending on the same float: no seed makes all 91 slots of a size
differ from all five, and the number that coincide is printed).  A set that misses a condition gets the next seed in
convolution_reference.CLASS_A_SEED."""
import numpy as np
import pytest

import convolution_reference as cr
import oracle as orc

f32 = np.float32
HOST_SIZES = [8, 9, 10, 21, 35, 44, 64, 75]


def oracle_slots(proj, ctf):
    """orc.convolve of every (o, c): conv [nO, nC, N, H, 2], sumC, sumsquareC [nO, nC]"""
    nO, nC = len(proj), len(ctf)
    conv = np.zeros((nO, nC) + proj.shape[1:], dtype=f32)
    sC, ssC = np.zeros((nO, nC), dtype=f32), np.zeros((nO, nC), dtype=f32)
    for o in range(nO):
        for c in range(nC):
            conv[o, c], sC[o, c], ssC[o, c] = orc.convolve(proj[o], ctf[c])
    return conv, sC, ssC


@pytest.mark.parametrize("N", HOST_SIZES)
def test_class_a_equals_the_oracle_bit_for_bit(N):
    a = cr.class_a(N)
    conv, sC, ssC = oracle_slots(a.proj, a.ctf)
    assert conv.tobytes() == a.conv.tobytes()
    assert sC.tobytes() == a.sumC.tobytes()
    assert ssC.tobytes() == a.sumsq.tobytes(), np.argwhere(ssC != a.sumsq)[:5]


@pytest.mark.parametrize("N", HOST_SIZES)
def test_class_b_against_the_oracle(N):
    """every bin of the oracle's spectrum within 2 * 2^-24 (|a b| + |c d|) of the exact product (two rounded products and
    one rounded sum); its sumC its first component; its sumsquareC the float32 chain over uncontracted terms of its own
    spectrum, bit for bit (the oracle is built with -ffp-contract=off)"""
    b = cr.class_b(N)
    conv, sC, ssC = oracle_slots(b.proj, b.ctf)
    u = 2.0 ** -24
    assert (np.abs(conv[..., 0].astype(np.float64) - b.re) <= 2 * u * b.mag_re).all()
    assert (np.abs(conv[..., 1].astype(np.float64) - b.im) <= 2 * u * b.mag_im).all()
    assert conv.tobytes() == cr.conv_f32(b.proj[:, None], b.ctf[None]).tobytes()
    assert sC.tobytes() == conv[:, :, 0, 0, 0].tobytes()
    assert ssC.tobytes() == cr.sumsquare_ordered(conv, N).tobytes()
    # and within the bound the device's sums are held to: a chain of M additions, the terms' and the division's roundings
    for o, c in [(0, 0), (3, 7), (6, 12)]:
        exact = cr.weighted_fsum(conv[o, c], N) / (N * N)
        assert abs(float(ssC[o, c]) - exact) <= (b.M + 3) * u * exact


# ---- the five wrong orders ----
def column_0_first(terms, N):
    H = N // 2 + 1
    jend = H - 1 if N % 2 == 0 else H
    row = [jend - 1] + list(range(jend - 1)) + ([H - 1] if N % 2 == 0 else [])
    idx = (np.arange(N)[:, None] * H + np.array(row)[None, :]).reshape(-1)
    return cr.chain_f32(terms[..., idx])


def reversed_order(terms, N):
    return cr.chain_f32(terms[..., ::-1])


def float4_pairwise(terms, N):
    """(x + y) + (z + w) added per 16-byte word, the tail one by one"""
    M = terms.shape[-1]
    q = terms[..., :M & ~3].reshape(terms.shape[:-1] + (-1, 4))
    words = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    return cr.chain_f32(np.concatenate([words, terms[..., M & ~3:]], axis=-1))


def tiles_swapped(terms, N):
    """the first two tiles of 960 terms in each other's place (sizes with more than two tiles)"""
    M, T = terms.shape[-1], cr.TILE_FUSED
    if M <= 2 * T:
        return None
    idx = np.concatenate([np.arange(T, 2 * T), np.arange(T), np.arange(2 * T, M)])
    return cr.chain_f32(terms[..., idx])


def tail_dropped(terms, N):
    M = terms.shape[-1]
    return cr.chain_f32(terms[..., :M - (M % 4 or 3)])


WRONG_ORDERS = [column_0_first, reversed_order, float4_pairwise, tiles_swapped, tail_dropped]


def test_the_wrong_orders_are_wrong_and_the_right_one_is_right():
    """on a hand-made chain: 2^26, then 3, 5, 2, 2 -- additions round to multiples of 8 once the sum is 2^26"""
    t = np.array([2.0 ** 26, 3, 5, 2, 2], dtype=f32)
    assert cr.chain_f32(t) == f32(2.0 ** 26 + 8)                 # + 3 -> down, + 5 -> up, + 2 -> down, + 2 -> down
    assert cr.chain_f32(t[::-1]) == f32(2.0 ** 26 + 16)          # 12 exactly, then 2^26 + 12: the tie goes to the even + 16
    assert float4_pairwise(t, 0) == f32(2.0 ** 26 + 8)           # (2^26 + 3 -> 2^26) + (5 + 2) -> + 8; then + 2 -> down
    assert tail_dropped(t, 0) == f32(2.0 ** 26 + 8) and tail_dropped(t[:4], 0) == f32(2.0 ** 26)
    bins, w = cr.parseval_order(4)                               # H = 3: per row column 1 doubled, column 0, column 2
    assert bins.tolist() == [1, 0, 2, 4, 3, 5, 7, 6, 8, 10, 9, 11] and w.tolist() == [2, 1, 1] * 4
    bins, w = cr.parseval_order(3)                               # H = 2: per row column 1 doubled, column 0
    assert bins.tolist() == [1, 0, 3, 2, 5, 4] and w.tolist() == [2, 1] * 3
    terms = np.arange(12, dtype=f32)
    assert column_0_first(terms[None], 4) == cr.chain_f32(terms[[1, 0, 2, 4, 3, 5, 7, 6, 8, 10, 9, 11]])


@pytest.mark.parametrize("N", cr.SIZES)
def test_every_class_a_case_tells_the_reference_order_from_five_wrong_ones(N):
    a = cr.class_a(N)
    assert a.distinct()
    assert len(set(a.place_orient)) == cr.N_ORIENT and len(set(a.place_ctf)) == cr.N_CTF
    assert not set(a.place_orient) & set(a.place_ctf)
    M = a.M
    special = [0, M - 1] + [p for p in (959, 960, 511, 512) if p < M]
    assert all(p in a.places for p in special), (special, a.places)
    assert any(p >= (M & ~3) - (0 if M % 4 else 3) for p in a.places)      # inside the last partial float4 / the last three
    assert cr.chain_f32(a.terms).tobytes() == a.chain.tobytes()
    coincide = {}
    for order in WRONG_ORDERS:
        wrong = order(a.terms, N)
        if wrong is None:
            assert M <= 1920
            continue
        differ = cr.divide_f32(wrong, N) != a.sumsq                         # [o, c]
        coincide[order.__name__] = int((~differ).sum())
        for nO, c0, nC in cr.shapes_of(N):
            assert differ[:nO, c0:c0 + nC].any(), (order.__name__, N, (nO, c0, nC), a.seed)
    print("N %d (seed %d): slots of %d whose sumsquareC a wrong order leaves unchanged: %s"
          % (N, a.seed, cr.N_ORIENT * cr.N_CTF, coincide))


def test_comparison_layout_by_hand_and_round_trip():
    """N = 8 as 2 x 4 (fast = 2, N1 = 2), H = 5, pitch 6: row pairs (0, 2), (4, 6), (1, 3), (5, 7), one pad word each"""
    spec = np.zeros((8, 5, 2), dtype=f32)
    for i in range(8):
        for j in range(5):
            spec[i, j] = (10 * i + j, -(10 * i + j) - 0.5)
    raw, data = cr.comparison_layout(spec, 2, 2, 6)
    want, mask = [], []
    for first, second in [(0, 2), (4, 6), (1, 3), (5, 7)]:
        for j in range(5):
            want += [spec[first, j], spec[second, j]]
            mask += [True, True]
        want += [(0, 0), (0, 0)]
        mask += [False, False]
    assert raw.shape == (48, 2) and raw.tolist() == np.array(want, dtype=f32).tolist() and data.tolist() == mask
    assert raw[0].tolist() == [0, -0.5] and raw[1].tolist() == [20, -20.5] and raw[12].tolist() == [40, -40.5]
    assert raw[25].tolist() == [30, -30.5] and raw[46].tolist() == [0, 0]
    rng = np.random.default_rng(3)
    for N, fast, N1, pad in [(8, 2, 2, 1), (8, 4, 1, 0), (8, 1, 4, 0), (64, 8, 4, 0), (192, 16, 6, 15), (9, 0, 0, 0)]:
        H = N // 2 + 1
        spec = rng.standard_normal((N, H, 2)).astype(f32)
        raw, data = cr.comparison_layout(spec, fast, N1, H + pad)
        assert data.sum() == N * H and raw.shape == (N * (H + pad), 2)
        assert cr.from_comparison_layout(raw, N, fast, N1, H + pad).tobytes() == spec.tobytes()
    raw, _ = cr.comparison_layout(spec, 0, 0, 5)
    assert raw.tobytes() == spec.tobytes()
