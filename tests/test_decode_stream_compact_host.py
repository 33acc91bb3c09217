"""CPU: a decode stream's compaction without a GPU (include/rlnc_hip.h, rlnc_decode_stream_compact) -- the symbol in the
header, the ctypes table and the library, the refusals that need no device, and the numpy model of the call with the
inputs that tests/test_gpu_decode_stream_compact.py runs on the device.

compact_model is built on true_rank_model (tests/test_true_rank_host.py): the kept slots u are the prefix's Ok slots.
The equivalence the call rests on is checked here on the CPU for every input family the GPU tests use: the model of the
kept vectors alone answers Ok for every one of them, has the prefix's rank, and its T is the prefix's T with the columns
gathered by u.  The same file asserts what every tested batch must hold, so that no GPU test can pass vacuously."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests import limit_shapes as ls
from tests.test_true_rank_host import NOT_USEFUL, OK, RECEIVED_ALL, sparse_vectors, true_rank_model

MUL = npo.mul_table()
# (5, 7) odd kd, m no multiple of 4; (16, 20) the form the default picks is the LDS one; (24, 67) B = 32, m no multiple
# of 4; (4, 1100) rows wider than 256 dwords; (300, 330) a scan and a list beyond one pass of 256 threads; (4, 8192) the
# most slots a stream takes: 32 statuses per thread of the scan, an e part of 2,048 dwords, slot indices up to 8,190
SHAPES = [(5, 7), (16, 20), (24, 67), (4, 1100), (300, 330), (4, 8192)]
NAMES = ["mixed", "chain", "late", "idle", "empty", "full", "sparse", "planted", "dense"]


def model_of(k, vectors):
    """true_rank_model, and the empty prefix."""
    if len(vectors) == 0:
        return [], 0, np.zeros((k, 0), np.uint8), None
    return true_rank_model(k, vectors)


def compact_model(k, co_prefix):
    """What rlnc_decode_stream_compact does with an object whose pushed slots hold the vectors co_prefix: (u, r, T, st)
    -- the kept slots u_0 < ... < u_{r-1} (the prefix's Ok slots), r = rank, T [k][r] the prefix's T with its columns
    gathered by u, and the prefix's statuses."""
    st, rank, T, _ = model_of(k, co_prefix)
    u = [t for t, s in enumerate(st) if s == OK]
    assert len(u) == rank
    return u, rank, np.ascontiguousarray(T[:, u]), st


@functools.lru_cache(maxsize=None)
def cases(k, m):
    """The batch of a shape: (co uint8 [9][m][k], done [9]) -- each object's coding vectors and how many of its slots
    are pushed before the compaction (a strict prefix: done < m), in the order of NAMES:
      mixed    dense with a zero piece, a duplicate and a multiple among the first slots
      chain    slot 0 zero and every later pushed slot useful: u_j = j + 1 throughout, the longest overwrite chain
      late     the first m - k slots zero, the others dense
      idle     independent vectors only: done == rank > 0
      empty    done == 0
      full     dense: rank k, then ReceivedAllPieces slots below done
      sparse   sparse_vectors at density 2
      planted  limit_shapes.planted: duplicates, multiples and sums of earlier pieces
      dense    dense random, pushed up to m - 2"""
    rng = np.random.default_rng(7000 * k + m)
    dense = lambda: rng.integers(1, 256, (m, k), dtype=np.uint8)  # noqa: E731
    mixed = dense()
    mixed[1] = 0
    mixed[3] = mixed[2]
    mixed[4] = MUL[0x1D][mixed[0]]
    chain = dense()
    chain[0] = 0
    late = dense()
    late[: m - k] = 0
    co = np.stack([mixed, chain, late, dense(), dense(), dense(), sparse_vectors(rng, k, m, 2), ls.planted(rng, k, m),
                   dense()])
    done = [m - 1, min(m - 1, k + 1), m - 1, max(1, k - 2), 0, m - 1, m - 1, m - 1, m - 2]
    co.setflags(write=False)
    return co, tuple(done)


@functools.lru_cache(maxsize=None)
def prefix_models(k, m):
    """compact_model of every object of cases(k, m), computed once."""
    co, done = cases(k, m)
    return tuple(compact_model(k, co[o, :done[o]]) for o in range(co.shape[0]))


@functools.lru_cache(maxsize=None)
def kept_models(k, m):
    """true_rank_model of every object's kept vectors alone, computed once."""
    co, _ = cases(k, m)
    return tuple(model_of(k, co[o][u]) for o, (u, _, _, _) in enumerate(prefix_models(k, m)))


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
