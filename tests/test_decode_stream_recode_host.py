"""CPU: a decode stream's recode without a GPU (include/rlnc_hip.h, rlnc_decode_stream_recode) -- the symbols in the
header, the ctypes table and the library, the plan size, the refusals that need no device, and, with the true-rank model
(tests/true_rank.py), that every named object of tests/recode_util.py has the rank, done and Ok list its name claims at
every shape tests/test_gpu_decode_stream_recode.py uses, so that no GPU test can pass vacuously."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.gpu_util import np_matmul
from tests.recode_util import FULL, NAMES, NOT_ENOUGH, REFUSAL_SHAPE, SHAPES, batch
from tests.stream_util import model_of
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL


@functools.lru_cache(maxsize=None)
def models(k, m, L, count):
    b = batch(k, m, L, count)
    return tuple(model_of(k, b.co[o, : b.done[o]]) for o in range(len(NAMES)))


def test_symbols_are_declared_bound_and_exported():
    from rlnc_amd import _lib, batch as rb

    lib = _lib.load()
    for s in ("rlnc_decode_stream_recode", "rlnc_decode_stream_recode_plan_bytes"):
        assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(lib, s)
    assert callable(getattr(rb.DecodeStream, "recode", None)) and callable(rb.stream_recode_plan_bytes)


def test_plan_bytes():
    from rlnc_amd import batch as rb

    pb = rb.stream_recode_plan_bytes
    # 0 exactly outside the limits: where the state is, and count 0 and 4,097
    for k, m, n in [(0, 8, 1), (8, 0, 1), (8, 8, 0), (4097, 4100, 1), (8, 8193, 1)]:
        assert pb(k, m, 4, n) == 0 and rb.state_bytes(k, m, n) == 0, (k, m, n)
    for k, m, n in [(1, 1, 1), (4096, 8192, 1), (4, 8192, 3), (300, 330, 9)]:
        assert rb.state_bytes(k, m, n) > 0
        assert pb(k, m, 0, n) == 0 and pb(k, m, 4097, n) == 0 and pb(k, m, 2 ** 40, n) == 0, (k, m, n)
        assert pb(k, m, 1, n) > 0 and pb(k, m, 4096, n) > 0, (k, m, n)
    for k, m, n, count in [(1, 1, 1, 1), (4096, 8192, 1, 4096), (4, 8192, 3, 5)] + [(k, m, 9, c) for k, m, _, c in SHAPES]:
        v = pb(k, m, count, n)
        assert v > 0 and v % 16 == 0, (k, m, n, count)
        # the expanded coefficients and 8 bytes per stream entry of whole row tiles, and the program's read-ahead
        tr = 8 if count <= 8 else 16 if count <= 16 else 32 if count <= 32 else 64
        assert v >= (n * count * m + 15) // 16 * 16 + n * -(-count // tr) * tr * m * 8 + 8 * tr
    # monotone in count, across every tile-size boundary, and in the other arguments
    for count in range(1, 200):
        assert pb(24, 40, count, 3) <= pb(24, 40, count + 1, 3), count
        assert pb(24, 40, count, 3) <= pb(24, 41, count, 3) and pb(24, 40, count, 3) <= pb(24, 40, count, 4), count
    assert pb(24, 40, 4095, 3) <= pb(24, 40, 4096, 3)
    for count in (1, 63, 64, 65, 1000, 4095):
        assert pb(4096, 8192, count, 2) <= pb(4096, 8192, count + 1, 2), count
    # k enters only through the limits
    assert pb(5, 40, 7, 3) == pb(24, 40, 7, 3)


def test_refusals_that_need_no_device():
    from rlnc_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    n = 10 ** 6
    f = lib.rlnc_decode_stream_recode
    assert f(None, p, n, p, 0, 16, 4, 20, 3, None, p, 4, p, p, p, p, n) == 100  # a null handle, before everything else
    assert b"ctx" in lib.rlnc_last_error()
    assert f(None, None, 0, None, 0, 0, 0, 0, 0, None, None, 0, None, None, None, None, 0) == 100
    assert b"ctx" in lib.rlnc_last_error()
    # k = 0 and L = 0 come next and need nothing of the handle (any non-null value)
    assert f(p, p, n, p, 0, 0, 4, 20, 3, None, p, 4, p, p, p, p, n) == 3   # PieceCountZero
    assert f(p, p, n, p, 0, 0, 0, 20, 3, None, p, 4, p, p, p, p, n) == 3   # ... before PieceLengthZero
    assert f(p, p, n, p, 0, 16, 0, 20, 3, None, p, 4, p, p, p, p, n) == 5  # PieceLengthZero
    assert f(p, p, n, p, 0, 16, 4, 20, 0, None, p, 4, p, p, p, p, n) == 0  # no objects: RLNC_OK, nothing launched
    assert f(p, p, n, p, 0, 16, 4, 20, 3, None, p, 0, p, p, p, p, n) == 0  # count 0: RLNC_OK, nothing launched


@pytest.mark.parametrize("k,m,L,count", SHAPES + [REFUSAL_SHAPE])
def test_every_object_is_what_its_name_claims(k, m, L, count):
    b = batch(k, m, L, count)
    n = len(NAMES)
    assert b.pieces.shape == (n, m, k + L) and b.src.shape == (n, k, L) and b.r.shape == (n, count, k)
    by = {name: (o, models(k, m, L, count)[o]) for o, name in enumerate(NAMES)}
    for name, (o, (st, rank, T, _)) in by.items():
        d = b.done[o]
        assert len(st) == d <= m, name
        assert rank == b.rank[o] and [t for t, s in enumerate(st) if s == OK] == list(b.useful[o]), name
        assert len(b.useful[o]) == rank, name
        if b.statuses[o] is not None:
            assert tuple(st) == b.statuses[o], name
        assert (rank == k) == (name in FULL or (name == "chain" and m > k)), name
        assert b.status[o] == (0 if rank else NOT_ENOUGH), name
        assert (b.expected[o] is None) == (rank == 0), name
        # the pushed slots are pieces of the object's source
        assert np.array_equal(b.pieces[o, :d, :k], b.co[o, :d]), name
        if d:
            assert np.array_equal(b.pieces[o, :d, k:], np_matmul(b.co[o, :d], b.src[o])), name
    o, (st, rank, T, _) = by["exact"]
    assert b.done[o] == k == rank and st == [OK] * k
    o, (st, rank, T, _) = by["padded"]
    assert b.done[o] > k and st[0] == NOT_USEFUL and st[-1] == OK
    assert st.count(NOT_USEFUL) == (3 if k >= 2 and m - k >= 3 else 2 if k >= 2 and m - k >= 2 else 1)
    assert not b.co[o, 0].any()  # the zero vector
    if k >= 2 and m - k >= 2:
        assert np.array_equal(b.co[o, 2], b.co[o, 1])  # the duplicate
        assert list(b.useful[o])[:2] == [1, 3]  # a gap in u between useful slots
    o, (st, rank, T, _) = by["chain"]
    assert st[0] == NOT_USEFUL and list(b.useful[o]) == list(range(1, b.done[o])) and rank == min(k, m - 1) >= 1
    o, (st, rank, T, _) = by["over"]
    assert b.done[o] > k and st[:k] == [OK] * k and set(st[k:]) == {RECEIVED_ALL}
    assert list(b.useful[o]) == list(range(k))  # the ReceivedAllPieces slots are left out
    o, (st, rank, T, _) = by["short"]
    assert rank == k - 1 == b.done[o]
    o, (st, rank, T, _) = by["deficient"]
    assert b.done[o] == m and rank == max(0, min(k - 1, m)) < k and (k == 1 or NOT_USEFUL in st)
    o, (st, rank, T, _) = by["empty"]
    assert b.done[o] == 0 and rank == 0
    o, (st, rank, T, _) = by["zeros-only"]
    assert b.done[o] > 0 and rank == 0 and not b.co[o, : b.done[o]].any() and set(st) == {NOT_USEFUL}
    o, (st, rank, T, _) = by["sparse"]
    assert (np.count_nonzero(b.co[o, :k], axis=1) == min(2, k)).all() and b.done[o] == k == rank
    # the random bytes hold zeros and nonzeros, and bytes from the rank on that a recode must ignore
    assert (b.r == 0).any() or count * k == 1
    assert b.r.any()


@pytest.mark.parametrize("k,m,L,count", SHAPES + [REFUSAL_SHAPE])
def test_the_expected_pieces_are_recoded_pieces_of_the_source(k, m, L, count):
    """A recoded piece is a coded piece: its data is its header times the source, and its header is r x co[u]."""
    b = batch(k, m, L, count)
    for o, name in enumerate(NAMES):
        e = b.expected[o]
        if e is None:
            continue
        u, rank = list(b.useful[o]), b.rank[o]
        assert e.shape == (count, k + L)
        assert np.array_equal(e[:, :k], np_matmul(b.r[o][:, :rank], b.co[o][u])), name
        assert np.array_equal(e[:, k:], np_matmul(e[:, :k], b.src[o])), name
