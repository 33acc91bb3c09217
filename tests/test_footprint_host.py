"""CPU: tests/footprint.py on numpy images -- the arena reports a stray or missing store at the right coordinates, and
passes a correct image.  This is what shows that the assertions of tests/test_gpu_footprint.py can fail on a store
outside the footprint, without moving a store's address on the GPU."""
import numpy as np
import pytest

from tests.footprint import MIN_GUARD, Arena, guard_bytes

N_OBJ, N_ROWS, N_IN, W, PAD = 2, 3, 13, 100, 5
ROW = 64 + W + PAD            # [64-byte header slot | data | pad]
OBJ = N_ROWS * ROW + 48       # a gap after every object


def coded_pieces_arena(base_off=1):
    """The layout of the strided matmul cases: hdr[o][i][0:n_in) in a 64-byte slot before each out[o][i][0:W)."""
    a = Arena((N_OBJ - 1) * OBJ + N_ROWS * ROW, seed=7, base_off=base_off, largest_row_stride=ROW)
    a.operand("hdr", 0, N_OBJ, OBJ, N_ROWS, ROW, N_IN)
    a.operand("out", 64, N_OBJ, OBJ, N_ROWS, ROW, W)
    rng = np.random.default_rng(8)
    a.expect("hdr", rng.integers(0, 256, (N_OBJ, N_ROWS, N_IN), dtype=np.uint8))
    a.expect("out", rng.integers(0, 256, (N_OBJ, N_ROWS, W), dtype=np.uint8))
    a.seal()
    return a


def good_image(a):
    return a.expected.copy()


def at(a, name, o, r, c):
    op = a.operands[name]
    return a.start + op.offset + o * op.obj_stride + r * op.row_stride + c


def test_layout_and_fill():
    a = coded_pieces_arena(base_off=15)
    assert a.guard >= MIN_GUARD and a.guard % 16 == 0 and a.start == a.guard + 15
    assert a.size == a.guard + 15 + (OBJ + N_ROWS * ROW) + a.guard
    assert guard_bytes(0) == MIN_GUARD and guard_bytes(10000) >= 20000
    assert int(a.mask.sum()) == N_OBJ * N_ROWS * (N_IN + W)
    assert not a.mask[: a.start].any() and not a.mask[a.end:].any()
    # the fill is not a constant, and after seal() no footprint byte's prefill equals its expected value
    assert np.unique(a.fill[: a.guard]).size > 200
    assert not (a.fill[a.mask] == a.expected[a.mask]).any()
    assert np.array_equal(a.fill[~a.mask], a.expected[~a.mask])


def test_correct_image_passes():
    a = coded_pieces_arena()
    assert a.find(good_image(a)) is None
    a.check(good_image(a))


@pytest.mark.parametrize("what,operand,o,r,c,kind", [
    ("row pad", "out", 1, 2, W + 3, "stray"),
    ("row pad, first byte past the row", "out", 0, 0, W, "stray"),
    ("header slot's unused tail", "hdr", 0, 1, N_IN, "stray"),
    ("header slot's last byte", "hdr", 1, 2, 63, "stray"),
    ("gap between the objects", "out", 0, N_ROWS - 1, W + PAD + 7, "stray"),
    ("first byte of the next object", "hdr", 1, 0, 0, "value"),
    ("first data byte of the next object", "out", 1, 0, 0, "value"),
    ("last byte of a row", "out", 0, 1, W - 1, "value"),
])
def test_flipped_byte_is_reported_where_it_is(what, operand, o, r, c, kind):
    a = coded_pieces_arena()
    img = good_image(a)
    off = at(a, operand, o, r, c)
    img[off] ^= 0x01
    f = a.find(img)
    assert f is not None and f.offset == off, what
    assert (f.kind, f.where, f.operand, f.obj, f.row, f.col) == (kind, "region", operand, o, r, c), (what, f)
    with pytest.raises(AssertionError) as ei:
        a.check(img)
    msg = str(ei.value)
    assert f"{operand}[object {o}][row {r}][column {c}]" in msg and "1 bytes differ" in msg
    assert ("stray write" in msg) == (kind == "stray")


@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("edge", ["near", "far"])
def test_flipped_guard_byte(side, edge):
    a = coded_pieces_arena()
    img = good_image(a)
    if side == "before":
        off = a.start - 1 if edge == "near" else 0
    else:
        off = a.end if edge == "near" else a.size - 1
    img[off] ^= 0x80
    f = a.find(img)
    assert f is not None and (f.kind, f.where, f.offset) == ("stray", "guard " + side, off)
    with pytest.raises(AssertionError, match="guard " + side):
        a.check(img)


@pytest.mark.parametrize("operand,o,r,c", [("out", 0, 0, 0), ("out", 1, 2, W - 1), ("hdr", 1, 1, N_IN - 1)])
def test_unwritten_byte_is_reported(operand, o, r, c):
    """A footprint byte the call never stored still holds its prefill, which seal() made differ from the value."""
    a = coded_pieces_arena()
    img = good_image(a)
    off = at(a, operand, o, r, c)
    img[off] = a.fill[off]
    f = a.find(img)
    assert f is not None and (f.kind, f.operand, f.obj, f.row, f.col) == ("value", operand, o, r, c)
    with pytest.raises(AssertionError, match="wrong or unwritten"):
        a.check(img)


def test_untouched_arena_fails_and_names_the_first_footprint_byte():
    a = coded_pieces_arena()
    f = a.find(a.fill.copy())  # a call that wrote nothing at all
    assert (f.kind, f.operand, f.obj, f.row, f.col) == ("value", "hdr", 0, 0, 0)


def test_status_arrays():
    """int32 [obj][m] statuses and int64 [obj] lengths as operands: little-endian bytes, one item per row."""
    nobj, m = 3, 5
    a = Arena(nobj * m * 4, seed=1)
    a.operand("piece_status", 0, nobj, m * 4, m, 4, 4)
    st = np.arange(nobj * m, dtype=np.int32).reshape(nobj, m) - 2
    a.expect("piece_status", st)
    a.seal()
    img = a.expected.copy()
    assert np.array_equal(img[a.start: a.end].view(np.int32).reshape(nobj, m), st)
    a.check(img)
    img[a.start + (2 * m + 3) * 4 + 1] ^= 0xFF
    f = a.find(img)
    assert (f.operand, f.obj, f.row, f.col) == ("piece_status", 2, 3, 1)
    b = Arena(nobj * 8, seed=2, base_off=0)
    b.operand("data_len", 0, 1, 0, nobj, 8, 8)
    b.expect("data_len", np.array([0, 1 << 40, 7], np.int64))
    b.seal()
    b.check(b.expected.copy())


def test_overlapping_operands_are_refused():
    a = Arena(256, seed=3)
    a.operand("x", 0, 1, 0, 2, 64, 40)
    with pytest.raises(AssertionError):
        a.operand("y", 32, 1, 0, 1, 0, 16)
    with pytest.raises(AssertionError):
        a.operand("z", 250, 1, 0, 1, 0, 16)  # past the region


# ---- the inputs of tests/test_gpu_footprint.py, checked without a GPU --------------------------------------------------
def test_matmul_case_grid_is_complete():
    """The pruned grid still holds every listed value, paired with every dispatch branch."""
    from tests.test_gpu_footprint import GAPS, MATMUL_CASES, OFFS, PADS

    assert 80 <= len(MATMUL_CASES) <= 130 and len({c.id for c in MATMUL_CASES}) == len(MATMUL_CASES)
    groups = {"stream": (1, 2, 3), "w1": (4, 8), "w2": (9, 16), "w4": (17, 32), "w8": (33, 64), "tiles": (65,)}
    for name, rows in groups.items():
        g = [c for c in MATMUL_CASES if c.n_out in rows and c.W >= 4096 and c.hdr and not c.zero]
        assert {c.n_out for c in g} == set(rows), name
        assert {c.pad for c in g} == set(PADS) and {c.off for c in g} == set(OFFS), name
        assert {c.gap for c in g} == set(GAPS), name
        assert {c.n_in for c in g} >= {1, 13} and {c.W for c in g} == {4096, 8192 + 16 + 3}, name
    narrow = [c for c in MATMUL_CASES if c.W < 4096 and c.hdr and not c.zero]
    assert {c.W for c in narrow} == {1, 15, 17, 4095} and {c.n_out for c in narrow} == {2, 5, 40}
    assert {c.n_in for c in narrow} == {3, 33} and {c.pad for c in narrow} == set(PADS)
    assert {c.off for c in narrow} == set(OFFS) and {c.gap for c in narrow} == set(GAPS)
    assert any(c.zero for c in MATMUL_CASES) and any(not c.hdr for c in MATMUL_CASES)


def test_decode_objects_are_what_they_are_built_to_be():
    """The constructed decode inputs: the oracle confirms the planned statuses and ranks (asserted inside
    decode_object), the complete object is complete, the deficient one has rank k - 1, zero T rows from its rank on and
    data length 0."""
    from tests.test_gpu_footprint import (DECODE_LENGTHS, DECODE_SHAPES, NOT_ALL_YET, NOT_USEFUL, OK, RECEIVED_ALL,
                                          decode_batch_objects, decode_object, in_tile_objects, scan_payloads)

    for k, m in DECODE_SHAPES:
        for L in DECODE_LENGTHS:
            full, useless, deficient = decode_batch_objects(k, m, L)
            assert full.rank == k and full.status == OK and full.data_len == k * L - 3
            assert (RECEIVED_ALL in full.statuses) == (m > k)
            assert useless.statuses.count(NOT_USEFUL) == 2 and useless.rank == min(k, m - 2)
            assert deficient.rank == k - 1 and deficient.status == NOT_ALL_YET and deficient.data_len == 0
            assert NOT_USEFUL in deficient.statuses and not deficient.T[k - 1:].any() and deficient.T[: k - 1].any()
            assert not deficient.decoded[k - 1:].any()
    for kind, k, m, L in [("complete", 5, 7, 4113), ("useless", 12, 16, 4096), ("deficient", 20, 24, 48),
                          ("complete", 40, 44, 8208)]:
        decode_object(kind, k, m, L)
    for L in (1023, 1024, 1025, 2055, 5000):
        pay, status, length = scan_payloads(L)
        assert pay.shape == (33, L) and len(set(length)) > 5
    objs = in_tile_objects(33)
    assert len(objs) == 33 and {o[3] for o in objs} == {0, 10, 11}
