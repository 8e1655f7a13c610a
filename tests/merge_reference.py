"""Exact reference of the merge of shards (k_merge_shards, bioem_hip_merge_host, bioem_hip_merge_topk_host_wide,
bioem_amd/dist_merge.py, the driver's merge): no product code, no numpy arithmetic on the values.

1. A map entry (Total_s, Constoadd_s, record_s) per shard s = 0 ... S-1, shards in ascending orientation-block order:

    Constoadd = max_s Constoadd_s                                                    exactly,
    winner    = the LOWEST s holding it (shard 0 when nothing was folded into any shard): its record is the result's,
    log P     = Constoadd + log sum_s Total_s e^(Constoadd_s - Constoadd)            in 256 bits.

   This is fold_reference.fold with rows = shards.  An angle-table entry (forAngles, ConstAngle) merges the same way and
   has no record.

   bound(entry): what the code does per shard, in double (u = 2^-53), is
       d_s = Constoadd_s - C*          one rounding: d_s is off by |d_s| u at most, which the exponential turns into a
                                       relative error of |d_s| u
       e_s = exp(d_s)                  within 2 ulp = 4 u
       x_s = Total_s * e_s             u
       tot += x_s                      S - 1 additions (the first one, 0 + x_0, is exact), u each on the running sum; all
                                       terms are positive, so every partial sum is at most the whole
   and nothing else (the maximum is a comparison, the record a copy).  To first order the relative error of the sum,
   which is the absolute error of its logarithm, is bounded by
       B = u [ sum_s w_s (|d_s| + 5) + S - 1 ],       w_s = Total_s e^(d_s) / sum, the exact share of term s.
   Below d_s = -708.39 the exponential is subnormal (or 0 below -745.13): its error is one subnormal spacing 2^-1074
   instead of 4 u of its value, so such a term adds 2^-1074 Total_s / sum.  The exact d_s and w_s are used (256 bits).

2. The K best orientations of WRITE_PROB_ANGLES.  The writer (bioem.cpp:1251-1286) walks the orientations in ascending
   order with a K-entry min-heap on (logp, orientation) and replaces the minimum when the minimum's logp is strictly
   below the newcomer's: writer_heap.  A full heap rejects the newest of equal keys and evicts the oldest when a larger
   key arrives.  With t the K-th largest key of a walk, the survivors are
       all keys above t, and the LAST m = K - #{keys > t} of the t-valued keys among the FIRST K keys >= t.
   A later walk over a longer list can shift that window of t-valued keys only towards earlier ones, never past the
   first K keys >= t.  So a shard offers its K survivors and, besides, the t-valued entries among its first K keys >= t
   that it did not keep: at most K - 1 more, a list of width 2K - 1 (shard_list).  The writer's loop over the union of
   such lists in orientation order (merge_lists) is the writer's loop over the whole table; K-wide lists are not enough.

The slips (keyword `slip`) exist to show that the host tests can tell them from the rule: "highest" (ties of Constoadd
to the highest shard), "le" (`<=` for `<` in the heap), and W = K in shard_list (K-wide lists)."""
import heapq
from collections import namedtuple

import mpmath

from fold_reference import MIN_PROB, PREC, U, fold, log_entry

SUBNORMAL = -708.39                    # exp(d) is subnormal below this d

MergedEntry = namedtuple("MergedEntry", "Constoadd winner logP")


def merge_entry(Total, Constoadd, slip=None):
    """Total[S], Constoadd[S] of one entry in shard order -> MergedEntry(Constoadd: float, winner: int, logP: mpf; -inf
    when every Total is 0)"""
    Total = [float(t) for t in Total]
    Constoadd = [float(c) for c in Constoadd]
    assert Total and len(Total) == len(Constoadd) and min(Constoadd) >= MIN_PROB
    r = fold(Constoadd, Total)
    winner = 0 if r.winner is None else r.winner           # None: every shard is fresh, the prior (0, MIN_PROB) stays
    if slip == "highest":
        winner = max(s for s, c in enumerate(Constoadd) if c == r.Constoadd)
    else:
        assert slip is None
    assert Constoadd[winner] == r.Constoadd
    return MergedEntry(r.Constoadd, winner, r.logP)


def bound(Total, Constoadd, prec=PREC):
    """B of the module text for one entry, as an mpf; 0 when every Total is 0 (the merged Total is then exactly 0)"""
    Total = [float(t) for t in Total]
    Constoadd = [float(c) for c in Constoadd]
    with mpmath.workprec(prec):
        C = mpmath.mpf(max(Constoadd))
        d = [mpmath.mpf(c) - C for c in Constoadd]
        terms = [mpmath.mpf(t) * mpmath.exp(x) for t, x in zip(Total, d)]
        total = mpmath.fsum(terms)
        if total == 0:
            return mpmath.mpf(0)
        B = mpmath.mpf(len(Total) - 1) * U
        for t, x, term in zip(Total, d, terms):
            B += term / total * (abs(x) + 5) * U
            if x < SUBNORMAL:
                B += mpmath.mpf(2) ** -1074 * mpmath.mpf(t) / total
        return B


def share(TotalOut, ConstoaddOut, Total, Constoadd, prec=PREC):
    """|log(TotalOut) + ConstoaddOut - log P| / B of a merged entry against its shards, as a float"""
    ref = merge_entry(Total, Constoadd)
    with mpmath.workprec(prec):
        return float(abs(log_entry(TotalOut, ConstoaddOut, prec) - ref.logP) / bound(Total, Constoadd, prec))


def writer_heap(logp, K, slip=None):
    """a K-entry min-heap of (logp, orientation) walked in orientation order; a newcomer replaces the minimum only when
    the minimum's logp is strictly below its own; emptied, the heap reads best first in descending (logp, orientation).
    logp: the keys by orientation index, or (key, orientation) pairs in ascending orientation."""
    assert slip in (None, "le")
    q = []
    for io, lp in enumerate(logp):
        if isinstance(lp, tuple):
            lp, io = lp
        if len(q) < K:
            heapq.heappush(q, (float(lp), io))
        elif q[0][0] < lp or (slip == "le" and q[0][0] <= lp):
            heapq.heapreplace(q, (float(lp), io))
    return sorted(q, reverse=True)


def shard_list(keys, o0, K, W):
    """the list of a shard that owns the orientations o0 ... o0 + len(keys) - 1: W entries (key, orientation) or None
    (unused).  Slots 0 ... K-1: the survivors of the shard's own walk, best first, by the closed rule of the module
    text (the host test compares them with writer_heap).  Slots K ... W-1 (W = 2K - 1): the other t-valued entries among
    the first K keys >= t, in ascending orientation."""
    assert W in (K, 2 * K - 1)
    items = [(float(k), o0 + i) for i, k in enumerate(keys)]
    if len(items) <= K:
        kept, extra = sorted(items, reverse=True), []
    else:
        t = sorted((k for k, _ in items), reverse=True)[K - 1]
        above = [x for x in items if x[0] > t]
        window = [x for x in [x for x in items if x[0] >= t][:K] if x[0] == t]      # t-valued among the first K keys >= t
        m = K - len(above)
        assert 1 <= m <= len(window)
        kept = sorted(above + window[len(window) - m:], reverse=True)
        extra = window[:len(window) - m]
    out = kept + [None] * (K - len(kept))
    if W > K:
        assert len(extra) <= K - 1
        out += extra + [None] * (K - 1 - len(extra))
    return out


def merge_lists(lists, K, slip=None):
    """the writer's loop over the union of the shards' lists in ascending orientation: (key, orientation) best first"""
    union = sorted((x for lst in lists for x in lst if x is not None), key=lambda x: x[1])
    assert len(set(o for _, o in union)) == len(union)
    return writer_heap(union, K, slip)
