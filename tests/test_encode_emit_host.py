"""CPU: the sender's emit without a GPU (include/rlnc_hip.h, rlnc_encode_emit) -- the symbols in the library and the
Python layer, the plan size, the checks that come before any device work, the Python argument asserts, and the numpy
model of tests/emit_util.py against a naive per-object loop on every named pattern and truncation point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import emit_util as eu
from tests.emit_util import emit_model, naive_split, pattern, split_model, truncation_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 100


@pytest.fixture(scope="module")
def lib():
    from rlnc_amd._lib import load

    return load()


def test_symbols_and_constant(lib):
    from rlnc_amd import _lib, batch

    for s in ("rlnc_encode_emit", "rlnc_encode_emit_plan_bytes"):
        assert hasattr(lib, s) and s in _lib._SIGS
    txt = open(os.path.join(ROOT, "include", "rlnc_hip.h")).read()
    assert re.search(r"#define\s+RLNC_EMIT_NONE\s+\((-\d+)\)", txt).group(1) == str(eu.NONE) == str(_lib.RLNC_EMIT_NONE)
    assert callable(batch.encode_emit_plan_bytes) and callable(batch.EncodeEmitter.emit)
    # the two comments name each other
    assert "rlnc_decode_stream_accept(arrivals_dev, object_dev, ..., count_dev)" in txt
    assert "What rlnc_encode_emit writes as" in txt


# ---- the model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(eu.PATTERNS))
def test_model_against_the_naive_loop(name):
    for nobj, cap in ((2 * eu.CHUNK + 3, 2), (2 * eu.CHUNK + 3, 5), (6, 16)):
        if name == "zero-runs" and nobj < 2 * eu.CHUNK + 3:
            continue
        want = pattern(name, nobj, cap)
        for n in truncation_points(want, cap):
            w, base, g, total, obj = split_model(want, cap, n)
            bases, granted, ntotal, nobjs = naive_split(want.tolist(), cap, n)
            assert base.tolist() == bases and g.tolist() == granted and total == ntotal, (name, nobj, cap, n)
            assert obj.tolist() == nobjs, (name, nobj, cap, n)
            assert (w == np.clip(want.astype(np.int64), 0, cap)).all() and total == min(int(w.sum()), n)


def test_patterns_are_what_their_names_say():
    nobj, cap = 2 * eu.CHUNK + 3, 7
    assert not pattern("all-zero", nobj, cap).any()
    assert (pattern("all-cap", nobj, cap) == cap).all()
    c = pattern("clamped", nobj, cap)
    assert (c < 0).any() and (c > cap).any() and eu.INT32_MIN in c and eu.INT32_MAX in c
    z = pattern("zero-runs", nobj, cap)
    nz = np.flatnonzero(z)
    assert len(nz) == 3 and (np.diff(nz) > eu.CHUNK).all()  # whole chunks of zeros between the emitting objects
    one = pattern("one-takes-all", nobj, cap)
    assert np.count_nonzero(one) == 1 and one.max() == cap
    last = pattern("last-only", nobj, cap)
    assert np.flatnonzero(last).tolist() == [nobj - 1]
    assert split_model(one, cap, cap)[3] == cap and split_model(one, cap, cap)[4].tolist() == [nobj // 2] * cap


def test_model_bytes_are_encode_batch_s():
    """A packet is r[i] || r[i] x src[o]: the C oracle's encode of object o over the coding vectors r[base_o ..]."""
    from oracle.oracle import Oracle

    orc = Oracle()
    rng = np.random.default_rng(3)
    k, L, n = 5, 37, 12
    src = rng.integers(0, 256, (4, k, L), dtype=np.uint8)
    r = rng.integers(0, 256, (n, k), dtype=np.uint8)
    want = np.array([3, 0, 9, 2], np.int32)
    out, obj, total, g = emit_model(src, want, r, 4)
    assert total == 9 and g.tolist() == [3, 0, 4, 2] and obj.tolist() == [0] * 3 + [2] * 4 + [3] * 2 + [eu.NONE] * 3
    at = 0
    for o in range(4):
        if g[o]:
            assert np.array_equal(out[at: at + g[o]], orc.encode(src[o], r[at: at + g[o]])), o
        at += int(g[o])
    out2, obj2, total2, g2 = emit_model(src, want, r[:8], 4)  # truncated inside object 3
    assert total2 == 8 and g2.tolist() == [3, 0, 4, 1] and np.array_equal(out2, out[:8])


# ---- the plan size ---------------------------------------------------------------------------------------------------

def test_plan_bytes_is_pure_aligned_and_monotonic(lib):
    f = lib.rlnc_encode_emit_plan_bytes
    ks = [1, 2, 15, 16, 17, 300, 4096]
    caps = [1, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 4095, 4096]
    objs = [1, 2, 1023, 1024, 1025, 65537, eu.MAX_OBJECTS]
    ns = [1, 2, 1024, eu.MAX_PACKETS]
    for k in ks:
        for cap in caps:
            row = [f(k, cap, o, 7) for o in objs]
            assert all(b > 0 and b % 16 == 0 for b in row) and row == sorted(row), (k, cap, row)
            assert row == [f(k, cap, o, 7) for o in objs]  # pure
    for o in (1, 1025):
        for cap in (3, 64):
            col = [f(k, cap, o, 7) for k in range(1, 70)]
            assert col == sorted(col)
        for k in (1, 16):
            col = [f(k, cap, o, 7) for cap in range(1, 200)] + [f(k, 4095, o, 7), f(k, 4096, o, 7)]
            assert col == sorted(col) and all(b % 16 == 0 for b in col), (k, o)
            col = [f(k, 8, o, n) for n in ns]
            assert col == sorted(col) and col[0] > 0
    # the streams: 8 bytes an entry of ceil(cap / tile rows) x k x tile rows per object, from cap = 4 on
    assert f(16, 4, 10, 5) - f(16, 3, 10, 5) == 10 * 8 * 16 * 8 + 512
    assert f(16, 70, 10, 5) - f(16, 3, 10, 5) == 10 * 128 * 16 * 8 + 512
    from rlnc_amd import batch

    assert batch.encode_emit_plan_bytes(16, 70, 10, 5) == f(16, 70, 10, 5)


def test_plan_bytes_is_zero_outside_each_limit(lib):
    f = lib.rlnc_encode_emit_plan_bytes
    good = dict(k=16, cap=8, nobj=5, n=40)
    limits = dict(k=eu.MAX_K, cap=eu.MAX_PER_OBJECT, nobj=eu.MAX_OBJECTS, n=eu.MAX_PACKETS)
    assert f(*good.values()) > 0
    for name, lim in limits.items():
        small = dict(good, k=1, cap=1) if name in ("nobj", "n") else good  # (keeps the sizes of this test small)
        assert f(*dict(small, **{name: lim}).values()) > 0, name
        assert f(*dict(small, **{name: lim + 1}).values()) == 0, name
        assert f(*dict(small, **{name: 0}).values()) == 0, name
        assert f(*dict(small, **{name: 2 ** 40}).values()) == 0, name


# ---- the checks before any device work ---------------------------------------------------------------------------------

def test_checks_without_a_device(lib):
    f = lib.rlnc_encode_emit
    assert f(None, None, 0, 4, 8, 1, None, 1, None, 1, None, 0, None, None, None, None, 0) == INVALID
    assert b"ctx" in lib.rlnc_last_error()


# ---- the Python argument asserts -------------------------------------------------------------------------------------

def _emitter(k, L, nobj, cap, n):
    """An emitter without its device plan buffer: the argument asserts come before any device work."""
    from rlnc_amd import batch

    e = batch.EncodeEmitter.__new__(batch.EncodeEmitter)
    e.k, e.L, e.num_objects, e.max_per_object, e.n, e.ctx, e._plan = k, L, nobj, cap, n, None, None
    return e


def test_constructor_asserts():
    from rlnc_amd import batch

    for bad in ((0, 8, 3, 2, 9), (4097, 8, 3, 2, 9), (4, 0, 3, 2, 9), (4, 8, 0, 2, 9), (4, 8, eu.MAX_OBJECTS + 1, 2, 9),
                (4, 8, 3, 0, 9), (4, 8, 3, 4097, 9), (4, 8, 3, 2, 0), (4, 8, 3, 2, eu.MAX_PACKETS + 1)):
        with pytest.raises(AssertionError, match="an emit takes"):
            batch.EncodeEmitter(*bad)


def test_emit_argument_asserts():
    import torch

    k, L, nobj, cap, n = 4, 8, 3, 2, 9
    e = _emitter(k, L, nobj, cap, n)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    good = dict(src=u8(nobj, k, L), want=i32(nobj), r=u8(n, k), out=u8(n, k + L), objects=i32(n), count=i32(1))
    bads = [
        dict(src=u8(nobj, k, L + 1)), dict(src=u8(nobj + 1, k, L)), dict(src=torch.zeros((nobj, k, L), dtype=torch.int8)),
        dict(src=u8(nobj, k, 2 * L)[:, :, ::2]),       # columns not dense
        dict(src=u8(nobj, 2 * k, L)[:, ::2]),          # rows not dense
        dict(r=u8(n, k + 1)), dict(r=u8(n - 1, k)), dict(r=u8(n, 2 * k)[:, ::2]),
        dict(out=u8(n, k + L + 1)), dict(out=u8(n - 1, k + L)), dict(out=u8(n, 2 * (k + L))[:, ::2]),
        dict(out=u8(k + L, n).t()),
    ]
    for bad in bads:
        with pytest.raises(AssertionError):
            e.emit(**dict(good, **bad))
    # strided operands the call takes pass the shape asserts and stop at the device one
    ok = dict(good, src=u8(nobj, k * L + 4096)[:, : k * L].view(nobj, k, L), out=u8(n, k + L + 37)[:, : k + L])
    with pytest.raises(AssertionError, match="device tensors required"):
        e.emit(**ok)
    with pytest.raises(AssertionError, match="device tensors required"):
        e.emit(**good)
    # the int32 operands, by name
    for name, bad in (("want", i32(nobj + 1)), ("want", torch.zeros(nobj, dtype=torch.int64)), ("objects", i32(n + 1)),
                      ("count", i32(2)), ("granted", i32(nobj - 1))):
        with pytest.raises(AssertionError, match=f"{name}: int32 contiguous device tensor"):
            e._i32(bad, {"want": (nobj,), "objects": (n,), "count": (1,), "granted": (nobj,)}[name], name)
