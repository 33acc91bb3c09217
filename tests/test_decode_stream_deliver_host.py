"""CPU: a decode stream's delivery without a GPU (include/rlnc_hip.h, rlnc_decode_stream_deliver) -- the symbols in the
header, the ctypes table and the library, the plan size, the refusals that need no device, and, with the true-rank model
(tests/true_rank.py), that every named object of tests/deliver_util.py has the rank, done and statuses its name claims at
every shape tests/test_gpu_decode_stream_deliver.py uses, so that no GPU test can pass vacuously.  For the rank-k objects
the model's T x the data rows of the pushed slots must be the source: what the device is asked to reproduce."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests.deliver_util import BAD_FORMAT, FULL, NAMES, NOT_ALL, REFUSAL_SHAPE, SHAPES, batch
from tests.gpu_util import np_matmul
from tests.stream_util import model_of
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL


@functools.lru_cache(maxsize=None)
def models(k, m, L):
    b = batch(k, m, L)
    return tuple(model_of(k, b.co[o, : b.done[o]]) for o in range(len(NAMES)))


def test_symbols_are_declared_bound_and_exported():
    from rlnc_amd import _lib, batch as rb

    lib = _lib.load()
    for s in ("rlnc_decode_stream_deliver", "rlnc_decode_stream_deliver_plan_bytes"):
        assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(lib, s)
    assert callable(getattr(rb.DecodeStream, "deliver", None)) and callable(rb.stream_deliver_plan_bytes)


def test_plan_bytes():
    from rlnc_amd import batch as rb

    pb = rb.stream_deliver_plan_bytes
    for k, m, n in [(0, 8, 1), (8, 0, 1), (8, 8, 0), (4097, 4100, 1), (8, 8193, 1)]:
        assert pb(k, m, n) == 0 and rb.state_bytes(k, m, n) == 0, (k, m, n)
    for k, m, n in [(1, 1, 1), (4096, 8192, 1), (4, 8192, 3), (300, 330, 9)] + [(k, m, 9) for k, m, _ in SHAPES]:
        v = pb(k, m, n)
        assert v > 0 and v % 16 == 0 and v >= n * k * m and rb.state_bytes(k, m, n) > 0, (k, m, n)
        # the T extract and 8 bytes per stream entry of whole row tiles, and the program's read-ahead of one source
        tr = 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64
        assert v >= (n * k * m + 15) // 16 * 16 + n * -(-k // tr) * tr * m * 8 + 8 * tr
    # non-decreasing in each argument, across every tile-size boundary of k
    for k in range(1, 140):
        assert pb(k, 40, 3) <= pb(k + 1, 40, 3) and pb(k, 40, 3) <= pb(k, 41, 3) and pb(k, 40, 3) <= pb(k, 40, 4), k
    for m in range(1, 70):
        assert pb(24, m, 3) <= pb(24, m + 1, 3), m
    assert pb(4095, 8191, 2) <= pb(4096, 8191, 2) <= pb(4096, 8192, 2) <= pb(4096, 8192, 3)


def test_refusals_that_need_no_device():
    from rlnc_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    n = 10 ** 6
    f = lib.rlnc_decode_stream_deliver
    assert f(None, p, n, p, 0, 16, 4, 20, 3, None, p, p, p, p, n) == 100  # a null handle, before everything else
    assert b"ctx" in lib.rlnc_last_error()
    assert f(None, None, 0, None, 0, 0, 0, 0, 0, None, None, None, None, None, 0) == 100
    assert b"ctx" in lib.rlnc_last_error()
    # k = 0 and L = 0 come next and need nothing of the handle (any non-null value)
    assert f(p, p, n, p, 0, 0, 4, 20, 3, None, p, p, p, p, n) == 3   # PieceCountZero
    assert f(p, p, n, p, 0, 0, 0, 20, 3, None, p, p, p, p, n) == 3   # ... before PieceLengthZero
    assert f(p, p, n, p, 0, 16, 0, 20, 3, None, p, p, p, p, n) == 5  # PieceLengthZero
    assert f(p, p, n, p, 0, 16, 4, 20, 0, None, p, p, p, p, n) == 0  # no objects: RLNC_OK, nothing launched


@pytest.mark.parametrize("k,m,L", SHAPES + [REFUSAL_SHAPE])
def test_every_object_is_what_its_name_claims(k, m, L):
    b = batch(k, m, L)
    assert b.pieces.shape == (len(NAMES), m, k + L) and b.src.shape == (len(NAMES), k, L)
    by = {n: (o, models(k, m, L)[o]) for o, n in enumerate(NAMES)}
    for name, (o, (st, rank, T, _)) in by.items():
        assert len(st) == b.done[o] <= m, name
        if b.rank[o] is not None:
            assert rank == b.rank[o] and tuple(st) == b.statuses[o], name
        assert (rank == k) == (name in FULL), name
        assert b.status[o] == (NOT_ALL if rank < k else BAD_FORMAT if name in ("badmarker", "zeros") else 0), name
        # the pushed slots are pieces of the object's source
        d = b.done[o]
        assert np.array_equal(b.pieces[o, :d, :k], b.co[o, :d]), name
    o, (st, rank, T, _) = by["exact"]
    assert b.done[o] == k and st == [OK] * k
    o, (st, rank, T, _) = by["padded"]
    assert b.done[o] > k and st[0] == NOT_USEFUL and st[-1] == OK  # rank k at the last slot, useless ones before it
    zero_cols = [t for t in range(b.done[o]) if not T[:, t].any()]
    assert zero_cols == [t for t, s in enumerate(st) if s == NOT_USEFUL]
    if k >= 2 and m - k >= 2:  # zero columns between nonzero ones
        assert any(0 < t and T[:, t - 1].any() and T[:, t + 1:].any() for t in zero_cols)
    o, (st, rank, T, _) = by["over"]
    assert b.done[o] > k and st[:k] == [OK] * k and set(st[k:]) == {RECEIVED_ALL}
    o, (st, rank, T, _) = by["short"]
    assert rank == k - 1 == b.done[o]
    o, (st, rank, T, _) = by["deficient"]
    assert b.done[o] == m and rank == max(0, min(k - 1, m)) < k
    o, (st, rank, T, _) = by["empty"]
    assert b.done[o] == 0 and rank == 0
    o, (st, rank, T, _) = by["sparse"]
    assert (np.count_nonzero(b.co[o, :k], axis=1) == min(2, k)).all() and b.done[o] == k
    # payloads: a different length per object (where k leaves room), the marker where the oracle puts it
    assert len(set(b.data_len)) == min(k, len(NAMES))
    for name, (o, _) in by.items():
        flat = b.src[o].reshape(-1)
        ok, n = npo.final_data_len(flat)
        if name == "zeros":
            assert not flat.any() and not ok
        elif name == "badmarker":
            assert flat[b.data_len[o]] == 0x80 and not flat[b.data_len[o] + 1:].any() and not ok
        else:
            assert ok and n == b.data_len[o] and flat[n] == 0x81, name
        assert b.length[o] == (b.data_len[o] if b.status[o] == 0 else 0), name


@pytest.mark.parametrize("k,m,L", SHAPES + [REFUSAL_SHAPE])
def test_the_models_transform_times_the_data_rows_is_the_source(k, m, L):
    b = batch(k, m, L)
    for o, name in enumerate(NAMES):
        st, rank, T, _ = models(k, m, L)[o]
        if name not in FULL:
            continue
        d = b.done[o]
        assert T.shape == (k, d)
        useful = [t for t in range(d) if T[:, t].any()]  # a zero column contributes nothing
        got = np_matmul(T[:, useful], b.pieces[o, useful, k:])
        assert np.array_equal(got, b.src[o]), name
