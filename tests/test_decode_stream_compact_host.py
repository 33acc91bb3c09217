"""CPU: a decode stream's compaction without a GPU (include/rlnc_hip.h, rlnc_decode_stream_compact) -- the symbol in the
header, the ctypes table and the library, the refusals that need no device, and the numpy model of the call
(tests/stream_util.py) with the inputs that tests/test_gpu_decode_stream_compact.py runs on the device.

compact_model is built on true_rank_model (tests/true_rank.py): the kept slots u are the prefix's Ok slots.
The equivalence the call rests on is checked here on the CPU for every input family the GPU tests use: the model of the
kept vectors alone answers Ok for every one of them, has the prefix's rank, and its T is the prefix's T with the columns
gathered by u.  The same file asserts what every tested batch must hold, so that no GPU test can pass vacuously."""
import ctypes as C

import numpy as np
import pytest

from tests.stream_util import NAMES, SHAPES, cases, kept_models, model_of, prefix_models
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL


def test_symbol_is_declared_bound_and_exported():
    from rlnc_amd import _lib, batch

    lib = _lib.load()
    s = "rlnc_decode_stream_compact"
    assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(lib, s)
    assert callable(getattr(batch.DecodeStream, "compact", None))


def test_null_arguments_are_refused_without_a_device():
    from rlnc_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    n = 10 ** 6
    assert lib.rlnc_decode_stream_compact(None, p, n, p, 0, 16, 4, 20, 3, p, p, p) == 100
    assert b"ctx" in lib.rlnc_last_error()
    assert lib.rlnc_decode_stream_compact(None, p, n, None, 0, 16, 0, 20, 3, None, None, None) == 100
    assert lib.rlnc_decode_stream_compact(None, None, 0, None, 0, 0, 0, 0, 0, None, None, None) == 100
    assert b"ctx" in lib.rlnc_last_error()


@pytest.mark.parametrize("k,m", SHAPES)
def test_the_kept_pieces_alone_give_the_gathered_state(k, m):
    """The equivalence, on the CPU: the model of the kept vectors has every status Ok, the prefix's rank, and T equal to
    the prefix's T with its columns gathered by u."""
    co, done = cases(k, m)
    for o, ((u, r, Tu, st), (st2, r2, T2, _)) in enumerate(zip(prefix_models(k, m), kept_models(k, m))):
        assert len(st) == done[o] < m, NAMES[o]
        assert st2 == [OK] * r and r2 == r, NAMES[o]
        assert T2.shape == (k, r) and np.array_equal(T2, Tu), NAMES[o]
        # a useless slot's column of T is zero: nothing is lost with it
        _, _, T, _ = model_of(k, co[o, :done[o]])
        assert not T[:, [t for t in range(done[o]) if t not in set(u)]].any(), NAMES[o]


@pytest.mark.parametrize("k,m", SHAPES)
def test_every_batch_holds_the_cases_the_gpu_tests_need(k, m):
    _, done = cases(k, m)
    by = dict(zip(NAMES, zip(prefix_models(k, m), done)))
    (u, r, _, st), d = by["mixed"]
    assert any(uj != j for j, uj in enumerate(u)) and st[1] == st[3] == st[4] == NOT_USEFUL and u[:3] == [0, 2, 5]
    (u, r, _, st), d = by["chain"]
    assert st[0] == NOT_USEFUL and u == list(range(1, d)) and r == d - 1 >= 2
    (u, r, _, st), d = by["late"]
    assert st[: m - k] == [NOT_USEFUL] * (m - k) and u and u[0] == m - k and d == m - 1
    (u, r, _, st), d = by["idle"]
    assert d == r > 0 and u == list(range(r))
    (u, r, _, st), d = by["empty"]
    assert d == 0 and r == 0 and u == []
    (u, r, _, st), d = by["full"]
    assert r == k and RECEIVED_ALL in st and len(st) == d
    (u, r, _, st), d = by["planted"]
    assert NOT_USEFUL in st and 0 < r
    (u, r, _, st), d = by["sparse"]  # something to reclaim: a useless slot, or slots answered at rank k
    assert 0 < r < d
    # the list of kept slots is longer than one pass of 256 threads, and so is the scan, where the shape allows
    if k > 256:
        assert max(r for (_, r, _, _), _ in by.values()) > 256 and max(done) > 256
