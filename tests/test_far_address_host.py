"""CPU: tests/far_address.py on numpy images -- an object written at a 32-bit-truncated offset and a byte flipped in
a far guard are reported at the right coordinates, and a correct set of images passes.  This is what shows that the
assertions of tests/test_gpu_far_address.py can fail, without truncating an address on the GPU."""
import numpy as np
import pytest

from tests.far_address import ARENA_BYTES, DELTA_ALIGNED, DELTA_ODD, FAR, FAR_ODD, NEAR, FarLayout
from tests.footprint import MIN_GUARD

N_ROWS, N_IN, W = 3, 5, 300
ROW = 64 + W + 4
BASE = 1 << 16


def far_layout(far=FAR):
    """Two objects of coded pieces (a header slot before each row), object 1 at `far`, and a near input."""
    rng = np.random.default_rng(3)
    lay = FarLayout(seed=11)
    lay.read("in", BASE + 8 * NEAR, 2, N_IN * W, N_IN, W, W, rng.integers(0, 256, (2, N_IN, W), dtype=np.uint8))
    lay.write("hdr", BASE, 2, far, N_ROWS, ROW, N_IN, rng.integers(0, 256, (2, N_ROWS, N_IN), dtype=np.uint8))
    lay.write("out", BASE + 64, 2, far, N_ROWS, ROW, W, rng.integers(0, 256, (2, N_ROWS, W), dtype=np.uint8))
    return lay.build()


def test_constants():
    assert FAR == 2**32 + DELTA_ALIGNED and FAR_ODD == 2**32 + DELTA_ODD
    assert DELTA_ALIGNED % 16 == 0 and DELTA_ODD % 2 == 1 and max(DELTA_ALIGNED, DELTA_ODD) < MIN_GUARD
    assert np.uint32(FAR & 0xFFFFFFFF) == DELTA_ALIGNED and np.int32(FAR & 0xFFFFFFFF) == DELTA_ALIGNED
    assert 3 * (2**31 + DELTA_ALIGNED) + (1 << 20) < ARENA_BYTES <= 8 << 30


def test_layout():
    lay = far_layout()
    assert len(lay.windows) == 3 and lay.guard >= MIN_GUARD and lay.guard >= 2 * ROW and lay.guard % 16 == 0
    w0, w_in, w1 = lay.windows
    assert w0.lo == BASE - lay.guard and w1.lo == BASE + FAR - lay.guard
    assert w0.hi - w0.lo == 2 * lay.guard + 2 * ROW + 64 + W
    assert int(w0.mask.sum()) == N_ROWS * (N_IN + W) == int(w1.mask.sum()) and not w_in.mask.any()
    assert lay.moved_bytes < 1 << 20
    for w in lay.windows:
        assert np.unique(w.fill[: lay.guard]).size > 200
        assert not (w.fill[w.mask] == w.expected[w.mask]).any()
        assert np.array_equal(w.fill[~w.mask], w.expected[~w.mask])
    # the truncated image of object 1 stays inside object 0's window
    assert BASE + DELTA_ALIGNED + 2 * ROW + 64 + W <= w0.hi


def test_correct_images_pass():
    lay = far_layout()
    assert lay.findings(lay.good_images()) == []
    lay.check(lay.good_images())


def test_a_window_outside_the_arena_is_refused():
    lay = FarLayout(seed=1)
    lay.write("out", 64, 2, FAR, 1, 0, 100, np.zeros((2, 1, 100), np.uint8))
    with pytest.raises(AssertionError, match="leaves the arena"):
        lay.build()  # no room for the guard before
    lay = FarLayout(seed=1)
    lay.write("out", BASE, 2, FAR, 1, 0, 100, np.zeros((2, 1, 100), np.uint8))
    lay.build()
    lay = FarLayout(seed=1)
    lay.write("out", BASE, 3, FAR, 1, 0, 100, np.zeros((3, 1, 100), np.uint8))
    with pytest.raises(AssertionError, match="leaves the arena"):
        lay.build()


@pytest.mark.parametrize("far,delta", [(FAR, DELTA_ALIGNED), (FAR_ODD, DELTA_ODD)], ids=["aligned", "odd"])
def test_object_written_at_the_truncated_offset_is_reported(far, delta):
    """What a kernel that computes o * obj_stride in 32 bits leaves behind: object 1's image delta bytes into object
    0's window, object 1's own window untouched."""
    lay = far_layout(far)
    imgs = lay.good_images()
    w0, _, w1 = lay.windows
    w1_image = imgs[2].copy()
    imgs[2] = w1.fill.copy()                       # never written
    for name in ("hdr", "out"):
        op = lay.operands[name]
        for r in range(op.n_rows):
            src = op.base + far + r * op.row_stride - w1.lo
            dst = op.base + delta + r * op.row_stride - w0.lo
            imgs[0][dst: dst + op.width] = w1_image[src: src + op.width]
    fs = lay.findings(imgs)
    assert [f.offset >= w1.lo for f in fs] == [False, True]
    damaged, unwritten = fs
    # object 0: the first wrong byte is object 1's header byte 0, delta bytes after object 0's
    assert damaged.offset == BASE + delta and damaged.obj == 0 and damaged.operand in ("hdr", "out")
    op = lay.operands[damaged.operand]
    assert op.base + damaged.row * op.row_stride + damaged.col == damaged.offset
    assert (unwritten.kind, unwritten.where, unwritten.operand, unwritten.obj, unwritten.row, unwritten.col) == \
        ("value", "region", "hdr", 1, 0, 0)
    with pytest.raises(AssertionError) as ei:
        lay.check(imgs)
    msg = str(ei.value)
    assert "hdr[object 1][row 0][column 0]" in msg and "[object 0]" in msg and "2 of 3 windows" in msg
    assert "wrong or unwritten byte" in msg


@pytest.mark.parametrize("side", ["before", "after"])
def test_flipped_byte_in_a_far_guard_is_reported(side):
    lay = far_layout()
    imgs = lay.good_images()
    w1 = lay.windows[2]
    i = 5 if side == "before" else (w1.hi - w1.lo) - 7
    imgs[2][i] ^= 0x80
    (f,) = lay.findings(imgs)
    assert f.kind == "stray" and f.offset == w1.lo + i and f.where == f"guard {side}"
    if side == "after":  # named by the last row before it
        assert (f.operand, f.obj, f.row) == ("out", 1, N_ROWS - 1) and f.col == f.offset - (BASE + 64 + FAR + 2 * ROW)
    with pytest.raises(AssertionError, match="stray write outside the footprint"):
        lay.check(imgs)


def test_flipped_input_byte_and_row_pad_are_reported():
    lay = far_layout()
    imgs = lay.good_images()
    imgs[1][lay.guard + W + 2] ^= 1            # in[0][1][2]
    imgs[2][lay.guard + 64 + W + 1] ^= 1       # out[1][0]'s pad
    a, b = lay.findings(imgs)
    assert (a.kind, a.operand, a.obj, a.row, a.col) == ("stray", "in", 0, 1, 2)
    assert (b.kind, b.operand, b.obj, b.row, b.col) == ("stray", "out", 1, 0, W + 1)
