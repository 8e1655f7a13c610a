"""CPU tests of the request helpers of bioem_amd.engine: _requests (an [n, k] integer array, a list of tuples or an array of
the request dtype, all to the same bytes) and _match_requests (the best records of a range of particles as requests).  No
handle and no device; every expected value is written out here."""
import struct

import numpy as np
import pytest

from bioem_amd import engine as eng

ROWS = [(3, 7, 1, -4, 5), (0, 2, 0, 31, -31), (9, 0, 2, 0, 0)]
# (dtype, the columns of ROWS it takes in the order of its fields)
DTYPES = [(eng.WINDOW_REQUEST_DTYPE, (0, 1, 2)), (eng.SCAN_REQUEST_DTYPE, (0, 1, 3, 4)),
          (eng.GRAD_REQUEST_DTYPE, (0, 1, 2, 3, 4))]


@pytest.mark.parametrize("dtype,cols", DTYPES)
def test_requests_from_every_form_are_the_same_bytes(dtype, cols):
    k = len(cols)
    assert dtype.itemsize == 4 * k and len(dtype.names) == k
    rows = [tuple(r[c] for c in cols) for r in ROWS]
    want = b"".join(struct.pack("<%di" % k, *r) for r in rows)   # packed int32, fields in column order
    typed = np.zeros(len(rows), dtype=dtype)
    for i, r in enumerate(rows):
        typed[i] = r
    for form in (np.array(rows, dtype=np.int64), np.array(rows, dtype=np.int32), rows, typed, typed.reshape(1, 3),
                 np.asfortranarray(np.array(rows, dtype=np.int32))):
        got = eng._requests(form, dtype)
        assert got.dtype == dtype and got.shape == (3,) and got.flags["C_CONTIGUOUS"]
        assert got.tobytes() == want
    assert eng._requests(typed[::2], dtype).tobytes() == want[:4 * k] + want[8 * k:]   # a strided view is packed


@pytest.mark.parametrize("dtype,cols", DTYPES)
def test_no_requests_are_an_empty_array_of_the_dtype(dtype, cols):
    for form in ([], np.zeros((0, len(cols)), dtype=np.int32), np.zeros(0, dtype=dtype)):
        got = eng._requests(form, dtype)
        assert got.dtype == dtype and got.shape == (0,)


@pytest.mark.parametrize("dtype,cols", DTYPES)
def test_a_wrong_column_count_raises(dtype, cols):
    k = len(cols)
    for wrong in (k - 1, k + 1):
        with pytest.raises(ValueError):
            eng._requests(np.zeros((k, wrong), dtype=np.int32), dtype)   # (k * wrong elements: k rows by size alone)
        with pytest.raises(ValueError):
            eng._requests(np.zeros((2, wrong), dtype=np.int32), dtype)
    with pytest.raises(ValueError):
        eng._requests(np.zeros((0, k + 1), dtype=np.int32), dtype)


def test_match_requests_of_a_range_of_records():
    pmap = np.zeros(5, dtype=eng.PROB_MAP_DTYPE)
    pmap["orient"] = [10, 11, 12, 13, 14]
    pmap["conv"] = [20, 21, 22, 23, 24]
    pmap["cent_x"] = [-1, -2, -3, -4, -5]
    pmap["cent_y"] = [6, 7, 8, 9, 5]
    pmap["Total"], pmap["norm"], pmap["mu"] = 1.5, 2.5, 3.5   # (no field of a request)
    w = eng._match_requests(pmap, 1, 4, eng.WINDOW_REQUEST_DTYPE)
    assert w.dtype == eng.WINDOW_REQUEST_DTYPE
    assert w.tolist() == [(1, 11, 21), (2, 12, 22), (3, 13, 23)]
    s = eng._match_requests(pmap, 1, 4, eng.SCAN_REQUEST_DTYPE)
    assert s.dtype == eng.SCAN_REQUEST_DTYPE
    assert s.tolist() == [(1, 11, -2, 7), (2, 12, -3, 8), (3, 13, -4, 9)]
    g = eng._match_requests(pmap, 1, 4, eng.GRAD_REQUEST_DTYPE)
    assert g.dtype == eng.GRAD_REQUEST_DTYPE
    assert g.tolist() == [(1, 11, 21, -2, 7), (2, 12, 22, -3, 8), (3, 13, 23, -4, 9)]
    assert eng._match_requests(pmap, 0, 5, eng.WINDOW_REQUEST_DTYPE).tolist() == [(p, 10 + p, 20 + p) for p in range(5)]
    assert eng._match_requests(pmap, 3, 3, eng.GRAD_REQUEST_DTYPE).shape == (0,)
    assert eng._match_requests(pmap, 4, 2, eng.SCAN_REQUEST_DTYPE).shape == (0,)
