"""CPU: a decode stream's accept without a GPU (include/rlnc_hip.h, rlnc_decode_stream_accept) -- the symbols in the
header, the ctypes table and the library, the plan size, the refusals that need no device, and that the model and every
named id pattern of tests/accept_util.py hold what their names claim, so that no test of
tests/test_gpu_decode_stream_accept.py can pass vacuously."""
import ctypes as C
import re

import numpy as np

from tests import accept_util as au
from tests.accept_util import ABSENT, CHUNK, FINISHED, NO_OBJECT, NO_ROOM, accept_model, host_loop, pattern, place


def test_symbols_are_declared_bound_and_exported():
    from rlnc_amd import _lib, batch as rb

    lib = _lib.load()
    for s in ("rlnc_decode_stream_accept", "rlnc_decode_stream_accept_plan_bytes"):
        assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(lib, s)
    assert callable(getattr(rb.DecodeStream, "accept", None)) and callable(getattr(rb.DecodeStream, "accept_reserve", None))
    assert callable(rb.stream_accept_plan_bytes)
    # the codes: in parentheses in the header, the same numbers in Python and in the model
    txt = open(_lib.HEADER_PATH).read()
    codes = dict(re.findall(r"#define\s+(RLNC_ACCEPT_\w+)\s+\((-\d+)\)", txt))
    assert {k: int(v) for k, v in codes.items()} == {
        "RLNC_ACCEPT_NO_ROOM": NO_ROOM, "RLNC_ACCEPT_NO_OBJECT": NO_OBJECT, "RLNC_ACCEPT_FINISHED": FINISHED,
        "RLNC_ACCEPT_ABSENT": ABSENT}
    for name, v in codes.items():
        assert getattr(_lib, name) == int(v)


def test_plan_bytes():
    from rlnc_amd import batch as rb

    pb = rb.stream_accept_plan_bytes
    assert pb(0, 5) == 0 and pb(5, 0) == 0 and pb(au.MAX_ARRIVALS + 1, 5) == 0 and pb(2 ** 40, 5) == 0
    assert pb(au.MAX_ARRIVALS, 1) > 0 and pb(1, 1) > 0
    for n in (1, 2, 3, 4, 5, 1023, 1024, 1025, 4097, 131074, au.MAX_ARRIVALS):
        for nobj in (1, 3, 4, 5, 256, 65537):
            v = pb(n, nobj)
            assert v > 0 and v % 16 == 0, (n, nobj)
            assert v >= 4 * (4 * n + nobj), (n, nobj)  # four int32 per arrival and one per object
            assert v <= pb(n, nobj + 1) and (n == au.MAX_ARRIVALS or v <= pb(n + 1, nobj)), (n, nobj)
    for n in range(1, 300):  # monotone across every rounding boundary
        assert pb(n, 7) <= pb(n + 1, 7) and pb(7, n) <= pb(7, n + 1), n


def test_refusals_that_need_no_device():
    from rlnc_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)  # never dereferenced: every call below returns before a launch
    big = 10 ** 6
    f = lib.rlnc_decode_stream_accept
    err = lib.rlnc_last_error

    def call(ctx=p, st=None, sn=0, arr=p, astride=0, obj=p, n=4, cnt=None, pc=p, stride=0, k=2, L=4, m=8, nobj=3, av=p,
             sl=p, rf=p, plan=p, pn=big):
        return f(ctx, st, sn, arr, astride, obj, n, cnt, pc, stride, k, L, m, nobj, av, sl, rf, plan, pn)

    assert call(ctx=None) == 100 and b"ctx" in err()  # a null handle, before everything else
    assert f(None, None, 0, None, 0, None, 0, None, None, 0, 0, 0, 0, 0, None, None, None, None, 0) == 100
    # k = 0 and L = 0 come next and need nothing of the handle (any non-null value)
    assert call(k=0) == 3 and call(k=0, L=0) == 3 and call(L=0) == 5
    assert call(n=0) == 0 and call(nobj=0) == 0  # nothing to do: RLNC_OK, nothing launched
    assert call(n=0, m=0, arr=None, plan=None) == 0
    # without a state the handle is not read before the launch: every refusal below names its limit and returns first
    assert call(m=0) == 100 and b"8192" in err()
    assert call(m=8193) == 100 and b"8192" in err()
    assert call(k=4097) == 100 and b"4096" in err()
    assert call(n=au.MAX_ARRIVALS + 1) == 100 and b"1048576" in err()
    assert call(astride=5) == 100 and b"arrival_stride" in err()  # below k + L = 6
    assert call(stride=8 * 6 - 1) == 100 and b"obj_stride" in err()
    for name in ("arr", "obj", "pc", "av"):
        assert call(**{name: None}) == 100, name
    need = lib.rlnc_decode_stream_accept_plan_bytes(4, 3)
    assert call(plan=None) == 100 and b"plan" in err()
    assert call(plan=C.c_void_p(p.value + 8)) == 100 and b"plan" in err()
    assert call(pn=need - 16) == 100 and b"plan" in err() and str(need).encode() in err()
    # the move grid: n x floor((k + L) / 4096) workgroups
    assert call(n=au.MAX_ARRIVALS, L=4096 * 2048, pn=2 ** 40) == 100 and b"workgroups" in err()


def test_the_model_is_the_host_loop():
    """The model's slots, applied, leave the pieces and the counts of INTEGRATION.md's loop of one copy per arrival."""
    rng = np.random.default_rng(5)
    for nobj, m, n in [(1, 1, 1), (3, 4, 30), (9, 7, 40), (5, 100, 3000)]:
        ids = rng.integers(0, nobj, n).astype(np.int32)
        avail = rng.integers(0, m + 1, nobj).astype(np.int32)
        arrivals = rng.integers(0, 256, (n, 6), dtype=np.uint8)
        pieces = rng.integers(0, 256, (nobj, m, 6), dtype=np.uint8)
        slot, av, refused = accept_model(ids, avail, m, nobj)
        want, filled = host_loop(pieces, arrivals, ids, avail, m)
        assert np.array_equal(place(pieces, arrivals, ids, slot), want) and av.tolist() == filled
        assert refused.sum() == (slot == NO_ROOM).sum() and (slot >= 0).sum() == (av - avail).sum()


def test_every_pattern_is_what_its_name_claims():
    k, L, m, nobj = au.ORDER_SHAPE
    assert k + L == 6 and m == 8192 and nobj == 3
    for n in (1023, 1024, 1025, 3000, 9000):
        ids = pattern(f"one-{n}")
        assert len(ids) == n and len(set(ids.tolist())) == 1 and 0 <= ids[0] < nobj
    assert len(pattern("one-9000")) > m
    slot, av, refused = accept_model(pattern("one-9000"), [0, 0, 0], m, nobj)
    assert (slot == NO_ROOM).sum() == 9000 - m == refused[1] and av[1] == m
    rr = pattern("round-robin")
    assert len(rr) > 2 * CHUNK and rr[:6].tolist() == [0, 1, 2, 0, 1, 2]
    s = pattern("sorted")
    assert len(s) > 2 * CHUNK and (np.diff(s) >= 0).all() and set(s.tolist()) == {0, 1, 2}
    r = pattern("reverse-sorted")
    assert len(r) > 2 * CHUNK and (np.diff(r) <= 0).all() and set(r.tolist()) == {0, 1, 2}
    sk = pattern("skewed")
    c = np.bincount(sk, minlength=3)
    assert len(sk) > 2 * CHUNK and c[0] > 0.8 * len(sk) and c[1] > 0 and c[2] > 0 and (np.diff(sk) != 0).any()
    assert pattern("single").tolist() == [1]
    # equal ids on both sides of a 1,024 boundary, and no other equal ids among the valid ones
    st = pattern("straddle")
    assert st[CHUNK - 1] == st[CHUNK] == 0 and st[2 * CHUNK - 1] == st[2 * CHUNK] == 1 and len(st) > 2 * CHUNK
    valid = np.flatnonzero((st >= 0) & (st < nobj))
    assert valid.tolist() == [5, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK] and st[5] == 2
    assert len(set(st.tolist())) == len(st) - 2  # the two pairs are the only duplicates at all
    slot, _, _ = accept_model(st, [7, 9, 11], m, nobj)
    assert slot[valid].tolist() == [11, 7, 8, 9, 10] and (np.delete(slot, valid) == NO_OBJECT).all()
    # in every pattern longer than a chunk some object has arrivals in more than one chunk
    for name in au.PATTERNS:
        ids = pattern(name)
        if len(ids) > CHUNK:
            assert any(len({i // CHUNK for i in np.flatnonzero(ids == o)}) > 1 for o in range(nobj)), name


def test_the_width_case_overflows_or_nearly_does():
    ids = au.width_ids()
    assert len(ids) == au.WIDTH_N == 40 and len(au.WIDTH_AVAIL) == au.WIDTH_OBJECTS == 9 and au.WIDTH_M == 7
    slot, av, refused = accept_model(ids, au.WIDTH_AVAIL, au.WIDTH_M, au.WIDTH_OBJECTS)
    assert (av >= au.WIDTH_M - 2).all(), av  # every object is full or within two slots of it
    assert (refused > 0).sum() >= 3 and (refused == 0).sum() >= 2 and (slot >= 0).sum() >= 15
    assert set(range(au.WIDTH_OBJECTS)) == set(ids.tolist())
    assert au.WIDTHS == [2, 15, 17, 4095, 4096, 4097, 8191, 12305]


def test_the_codes_case_holds_every_code():
    ids, avail, m, nobj, count, finished = au.codes_case()
    assert avail.tolist() == [-5, 0, m - 1, m, m + 3]
    assert {-1, nobj, au.INT32_MIN, au.INT32_MAX} <= set(ids.tolist())
    slot, av, refused = accept_model(ids, avail, m, nobj, count, finished)
    assert {NO_ROOM, NO_OBJECT, FINISHED, ABSENT} <= set(slot.tolist()) and (slot >= 0).any()
    assert (slot[count:] == ABSENT).all() and (slot[:count] != ABSENT).all() and 0 < count < len(ids)
    assert refused[2] == 2 and av[2] == m  # an object that overflows
    assert 4 not in ids[:count].tolist() and av[4] == m and refused[4] == 0  # no arrival: avail rewritten, clamped
    assert av[0] == 3 and av[1] == avail[1] and refused[1] == 0  # clamped from below; finished: as it was
    assert (slot[ids == 1][: (ids[:count] == 1).sum()] == FINISHED).all()
    # without the state nothing is finished, and count beyond n, 0 and negative
    slot2, av2, _ = accept_model(ids, avail, m, nobj)
    assert FINISHED not in slot2 and ABSENT not in slot2 and av2[1] == (ids == 1).sum()
    assert np.array_equal(accept_model(ids, avail, m, nobj, len(ids) + 5)[0], slot2)
    for c in (0, -2):
        s, a, r = accept_model(ids, avail, m, nobj, c)
        assert (s == ABSENT).all() and a.tolist() == [0, 0, m - 1, m, m] and not r.any()
