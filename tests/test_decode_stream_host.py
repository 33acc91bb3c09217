"""CPU: the decode stream's interface without a GPU (include/rlnc_hip.h, "Decode streams") -- its four symbols in the
header, the ctypes table and the library, the state size against rlnc_decode_large_workspace_bytes over the shapes of
tests/limit_shapes.py, and the argument checks that need no device."""
import ctypes as C
import re

import pytest

from tests import limit_shapes as ls

SYMBOLS = ["rlnc_decode_stream_init", "rlnc_decode_stream_push", "rlnc_decode_stream_snapshot",
           "rlnc_decode_stream_state_bytes"]
INSIDE = sorted({(k, m) for k, m, _, _ in ls.LARGE_NARROW} | set(ls.LARGE_OTHER) | {(1, 1), (4096, 1), (1, 8192)})
OUTSIDE = [(0, 8), (8, 0), (4097, 8192), (4096, 8193), (2 ** 31, 8), (8, 2 ** 31), (2 ** 40, 2 ** 40)]


def test_symbols_are_declared_bound_and_exported():
    from rlnc_amd import _lib

    lib = _lib.load()
    declared = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib._SIGS, s
        assert hasattr(lib, s), s
    assert re.search(r"#define\s+RLNC_STATUS_PENDING\s+\(-1\)", open(_lib.HEADER_PATH).read())
    assert _lib.RLNC_STATUS_PENDING == -1


def test_state_bytes_against_the_large_workspace():
    from rlnc_amd import batch

    for k, m in INSIDE:
        assert ls.large_block(k, m) > 0
        one = batch.state_bytes(k, m, 1)
        assert one > 0 and one % 16 == 0, (k, m)
        assert one >= batch.decode_large_workspace_bytes(k, m, 1), (k, m)
        for n in (2, 3, 1000):  # linear in the number of objects
            assert batch.state_bytes(k, m, n) == n * one, (k, m, n)
            assert batch.state_bytes(k, m, n) >= batch.decode_large_workspace_bytes(k, m, n)
    for k, m in OUTSIDE:
        assert batch.decode_large_workspace_bytes(k, m, 1) == 0 and batch.state_bytes(k, m, 1) == 0, (k, m)
    for k, m in INSIDE[:4]:  # the object count: zero, and more than a grid can take
        for n in (0, 2 ** 31):
            assert batch.decode_large_workspace_bytes(k, m, n) == 0 and batch.state_bytes(k, m, n) == 0, (k, m, n)
    # zero exactly where the workspace is, across the edges of both limits
    for k in (1, 4095, 4096, 4097):
        for m in (1, 8191, 8192, 8193):
            assert (batch.state_bytes(k, m, 2) == 0) == (batch.decode_large_workspace_bytes(k, m, 2) == 0), (k, m)


def test_null_arguments_are_refused_without_a_device():
    from rlnc_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    n = 10 ** 6
    assert lib.rlnc_decode_stream_init(None, p, n, 16, 20, 3) == 100
    assert lib.rlnc_decode_stream_init(None, None, 0, 16, 20, 3) == 100
    assert lib.rlnc_decode_stream_push(None, p, n, p, 0, 16, 4, 20, 3, p, 20, None, None) == 100
    assert lib.rlnc_decode_stream_push(None, None, 0, None, 0, 0, 0, 0, 0, None, 0, None, None) == 100
    assert lib.rlnc_decode_stream_snapshot(None, p, n, 16, 20, 3, None, None, None) == 100
    assert lib.rlnc_decode_stream_snapshot(None, None, 0, 16, 20, 3, p, p, p) == 100
    assert b"ctx" in lib.rlnc_last_error()


def test_decode_stream_refuses_a_shape_outside_the_limits_before_anything_else():
    from rlnc_amd import batch

    with pytest.raises(AssertionError):
        batch.DecodeStream(4097, 8192, 1)
