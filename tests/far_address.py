"""Far-address windows: does a device call address its operands with 64 bits?

One device arena of ARENA_BYTES = 3 * 2^31 + 2^26 uninitialised bytes (6.06 GiB, `torch.empty`; the largest case is
four output rows at a stride of 2^31 + delta) is shared by every far test of a module.  The operands of a call are
*windows* into it: each operand is [n_obj][n_rows] rows of `width` bytes at a byte offset and strides of any magnitude;
the rows of all operands of a call are clustered (rows closer than 1 MiB share a window), and every cluster becomes one
window `guard | rows | guard` with a guard of at least 8 KiB and two of the call's near row strides (tests/footprint.py's
rule; a stride of 1 MiB or more separates windows and needs no guard of its size).  Only the windows travel: each is
prefilled on the host from a seeded generator (never a constant), inputs hold their data, every byte the call should
write is prefilled to differ from its expected value; after the call the windows are read back, the written bytes must
equal the numpy / oracle image and every other byte of every window -- inputs, pads, guards -- its prefill.  The first
offender is named as (operand, object, row, column).  The arena itself is never uploaded or read back.

The far stride is FAR = 2^32 + delta with delta below the guard: DELTA_ALIGNED = 4096 + 16, DELTA_ODD = 4096 + 1.  An
offset of o * FAR that some kernel truncated to 32 bits, signed or unsigned, is o * delta: object 1's rows then land
delta bytes into object 0's window -- its rows and its guard after, both inside the arena -- and the check reports
object 0 damaged and object 1 unwritten.  A wrong address of that kind is never outside the allocation, which is what
makes a failing far test (and a library built with such a truncation on purpose) harmless on a shared device.  (The one
case this does not cover is a row stride of 2^31 + delta truncated to a *signed* 32 bits, which is negative: the arena
would have to be 8 GiB for it.)

Everything but `FarArena` is numpy on host arrays (tests/test_far_address_host.py runs it without a GPU).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.footprint import MIN_GUARD, Finding

FAR = (1 << 32) + 4096 + 16
DELTA_ALIGNED = 4096 + 16
DELTA_ODD = 4096 + 1
FAR_ODD = (1 << 32) + DELTA_ODD
ARENA_BYTES = 3 * (1 << 31) + (1 << 26)
NEAR = 1 << 20  # rows further apart than this are in windows of their own


@dataclass(frozen=True)
class FarOperand:
    name: str
    base: int        # arena offset of [0][0][0]
    n_obj: int
    obj_stride: int
    n_rows: int
    row_stride: int
    width: int
    written: bool

    def row_starts(self) -> np.ndarray:
        """Arena offsets of the rows, [n_obj][n_rows]."""
        return (self.base + np.arange(self.n_obj, dtype=np.int64)[:, None] * self.obj_stride +
                np.arange(self.n_rows, dtype=np.int64)[None, :] * self.row_stride)


@dataclass
class Window:
    lo: int                 # arena offsets [lo, hi)
    hi: int
    fill: np.ndarray
    expected: np.ndarray
    mask: np.ndarray       # bytes the call writes
    inputs: np.ndarray     # bytes the call reads (an in-place output's bytes are in both)


class FarLayout:
    """The windows of one call.  Lay the operands out (`read` / `write`), then `build`; `upload` before the call,
    `check(readback(...))` after it."""

    def __init__(self, seed: int, arena_bytes: int = ARENA_BYTES):
        self.seed = seed
        self.arena_bytes = int(arena_bytes)
        self.operands: dict[str, FarOperand] = {}
        self.values: dict[str, np.ndarray] = {}
        self.windows: list[Window] = []
        self.guard = MIN_GUARD

    # ---- layout ------------------------------------------------------------------------------------------------------
    def _add(self, name, base, n_obj, obj_stride, n_rows, row_stride, width, values, written):
        assert name not in self.operands and not self.windows
        op = FarOperand(name, int(base), int(n_obj), int(obj_stride), int(n_rows), int(row_stride), int(width), written)
        v = np.ascontiguousarray(values).view(np.uint8).reshape(op.n_obj, op.n_rows, op.width)
        self.operands[name] = op
        self.values[name] = v
        return op

    def read(self, name, base, n_obj, obj_stride, n_rows, row_stride, width, values):
        """An input: the windows hold `values` ([n_obj][n_rows][width] bytes) before the call and after it."""
        return self._add(name, base, n_obj, obj_stride, n_rows, row_stride, width, values, False)

    def write(self, name, base, n_obj, obj_stride, n_rows, row_stride, width, values):
        """An output: the call must leave `values` in exactly these bytes."""
        return self._add(name, base, n_obj, obj_stride, n_rows, row_stride, width, values, True)

    def build(self) -> "FarLayout":
        near = [op.row_stride for op in self.operands.values() if op.n_rows > 1 and 0 < abs(op.row_stride) < NEAR]
        self.guard = (max([MIN_GUARD] + [2 * abs(s) for s in near]) + 15) // 16 * 16
        spans = sorted((int(r), int(r) + op.width) for op in self.operands.values() for r in op.row_starts().reshape(-1))
        clusters = [list(spans[0])]
        for lo, hi in spans[1:]:
            if lo - clusters[-1][1] < NEAR:
                clusters[-1][1] = max(clusters[-1][1], hi)
            else:
                clusters.append([lo, hi])
        rng = np.random.default_rng(self.seed)
        for lo, hi in clusters:
            lo, hi = lo - self.guard, hi + self.guard
            assert 0 <= lo and hi <= self.arena_bytes, f"window [{lo}, {hi}) leaves the arena of {self.arena_bytes}"
            assert not self.windows or self.windows[-1].hi <= lo
            fill = rng.integers(0, 256, hi - lo, dtype=np.uint8)
            self.windows.append(Window(lo, hi, fill, fill.copy(), np.zeros(hi - lo, bool), np.zeros(hi - lo, bool)))
        for written in (False, True):  # inputs first: an in-place output's expectation replaces its input
            for op in self.operands.values():
                if op.written != written:
                    continue
                v = self.values[op.name]
                for o in range(op.n_obj):
                    for r in range(op.n_rows):
                        a = int(op.base + o * op.obj_stride + r * op.row_stride)
                        w = self._window_of(a)
                        sl = slice(a - w.lo, a - w.lo + op.width)
                        if written:
                            assert not w.mask[sl].any(), f"{op.name}: footprint overlaps"
                            w.mask[sl] = True
                            w.expected[sl] = v[o, r]
                        else:
                            w.fill[sl] = v[o, r]
                            w.expected[sl] = v[o, r]
                            w.inputs[sl] = True
        for w in self.windows:  # an unwritten byte can never pass by coincidence (in place: the prefill is the input)
            same = w.mask & ~w.inputs & (w.fill == w.expected)
            w.fill[same] ^= 0x5A
        return self

    def _window_of(self, off: int) -> Window:
        for w in self.windows:
            if w.lo <= off < w.hi:
                return w
        raise AssertionError(f"arena offset {off} is in no window")

    @property
    def moved_bytes(self) -> int:
        return sum(w.hi - w.lo for w in self.windows)

    # ---- device ------------------------------------------------------------------------------------------------------
    def upload(self, arena) -> None:
        import torch

        for w in self.windows:
            assert w.hi <= arena.size, f"window [{w.lo}, {w.hi}) leaves the arena of {arena.size}"
            arena.t[w.lo: w.hi].copy_(torch.from_numpy(w.fill))
        torch.cuda.synchronize()

    def readback(self, arena) -> list:
        import torch

        torch.cuda.synchronize()
        return [arena.t[w.lo: w.hi].cpu().numpy() for w in self.windows]

    def ptr(self, arena, name) -> int:
        return arena.ptr + self.operands[name].base

    # ---- the check (pure numpy) --------------------------------------------------------------------------------------
    def locate(self, off: int):
        """(where, operand, object, row, column) of an arena offset inside a window: the row that starts closest before
        it (of a written operand, if two start alike)."""
        w = self._window_of(off)
        best = None
        for op in self.operands.values():
            starts = op.row_starts()
            for o in range(op.n_obj):
                for r in range(op.n_rows):
                    s = int(starts[o, r])
                    if w.lo <= s <= off and (best is None or (off - s, not op.written) < best[0]):
                        best = ((off - s, not op.written), op.name, o, r)
        if best is None:
            return "guard before", None, None, None, None
        where = "region"
        if off >= w.hi - self.guard and not w.mask[off - w.lo]:
            where = "guard after"
        return where, best[1], best[2], best[3], best[0][0]

    def findings(self, images) -> list:
        """The first byte of each window's image that is not what the footprint allows (windows in arena order)."""
        out = []
        assert len(images) == len(self.windows)
        for w, img in zip(self.windows, images):
            img = np.asarray(img, np.uint8).reshape(-1)
            assert img.size == w.hi - w.lo
            bad = np.flatnonzero(img != w.expected)
            if bad.size == 0:
                continue
            i = int(bad[0])
            where, name, o, r, c = self.locate(w.lo + i)
            out.append(Finding("value" if w.mask[i] else "stray", where, name, o, r, c, w.lo + i, int(img[i]),
                               int(w.expected[i])))
        return out

    def check(self, images) -> None:
        fs = self.findings(images)
        if fs:
            n = sum(int(np.count_nonzero(np.asarray(img, np.uint8).reshape(-1) != w.expected))
                    for w, img in zip(self.windows, images))
            where = "; ".join(str(f) if f.where == "region" or f.operand is None else
                              f"{f}, {f.col} bytes from the start of {f.operand}[object {f.obj}][row {f.row}]" for f in fs)
            raise AssertionError(f"{where} ({n} bytes differ in {len(fs)} of {len(self.windows)} windows)")

    def good_images(self) -> list:
        return [w.expected.copy() for w in self.windows]


class FarArena:
    """The module's one device allocation; its contents are never defined outside the windows a test uploaded."""

    def __init__(self, nbytes: int = ARENA_BYTES, device="cuda:0"):
        import torch

        self.t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self.ptr = self.t.data_ptr()
        self.size = int(nbytes)
        assert self.ptr % 256 == 0

    def run(self, layout: FarLayout, call) -> None:
        """Uploads the windows, makes the call, reads the windows back and checks them."""
        layout.upload(self)
        call()
        layout.check(layout.readback(self))

    def strided(self, layout: FarLayout, name):
        """The operand as a strided torch view [n_obj][n_rows][width] of the arena."""
        op = layout.operands[name]
        return self.t.as_strided((op.n_obj, op.n_rows, op.width), (op.obj_stride, op.row_stride, 1), op.base)
