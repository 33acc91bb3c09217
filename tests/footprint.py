"""Footprint arenas: does a device call write exactly the bytes it documents?

An Arena is one uint8 buffer laid out `guard | region | guard` and filled from a seeded numpy generator (never a
constant: a stray store of that constant would pass).  The outputs of a call ("operands") are placed in the region at
chosen byte offsets and strides; each operand marks, in a boolean mask over the host image, exactly the bytes the call
documents as written (`[o][i][0:width)` at the given strides), and records what they must hold.  After the call the
whole arena is read back and `check` compares it: every masked byte equals the expected image, every other byte of the
arena -- row pads, header-slot tails, gaps between objects, both guards -- still holds its prefill.  The first offending
byte is named as (operand, object, row, column) or "guard before" / "guard after".

Everything here is numpy on host arrays; torch is imported only by `Arena.device` and `assert_inputs_unchanged`
(tests/test_footprint_host.py exercises the rest without a GPU).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MIN_GUARD = 8192


def guard_bytes(largest_row_stride: int = 0) -> int:
    """max(8 KiB, two of the largest row strides), rounded up to 16: a store one whole row or one 4 KiB column block
    astray still lands inside the allocation."""
    return (max(MIN_GUARD, 2 * int(largest_row_stride)) + 15) // 16 * 16


@dataclass(frozen=True)
class Operand:
    name: str
    offset: int      # bytes from the region's start
    n_obj: int
    obj_stride: int
    n_rows: int
    row_stride: int
    width: int       # bytes written per row

    def offsets(self) -> np.ndarray:
        """Region-relative byte offsets of the footprint, shape [n_obj][n_rows][width]."""
        return (self.offset + np.arange(self.n_obj, dtype=np.int64)[:, None, None] * self.obj_stride +
                np.arange(self.n_rows, dtype=np.int64)[None, :, None] * self.row_stride +
                np.arange(self.width, dtype=np.int64)[None, None, :])

    @property
    def extent(self) -> int:
        return (self.n_obj - 1) * self.obj_stride + (self.n_rows - 1) * self.row_stride + self.width


@dataclass(frozen=True)
class Finding:
    kind: str        # "value" (a masked byte is wrong or unwritten) or "stray" (a byte outside the footprint changed)
    where: str       # "guard before", "guard after" or "region"
    operand: str | None
    obj: int | None
    row: int | None
    col: int | None  # >= the operand's width: the row's pad (or whatever follows the row)
    offset: int      # arena offset of the byte
    got: int
    want: int

    def __str__(self):
        what = ("wrong or unwritten byte" if self.kind == "value" else "stray write outside the footprint")
        if self.where != "region":
            place = self.where
        elif self.operand is None:
            place = "region byte outside every operand"
        else:
            place = f"{self.operand}[object {self.obj}][row {self.row}][column {self.col}]"
        return f"{what} at {place} (arena offset {self.offset}): got 0x{self.got:02X}, want 0x{self.want:02X}"


class Arena:
    """guard | base_off | region | guard.  `base_off` (0..15) is the region's offset from a 16-byte boundary (the arena's
    device allocation and `guard` are multiples of 16)."""

    def __init__(self, region_bytes: int, *, seed: int, base_off: int = 0, largest_row_stride: int = 0):
        assert 0 <= base_off < 16 and region_bytes > 0
        self.guard = guard_bytes(largest_row_stride)
        self.start = self.guard + base_off
        self.end = self.start + int(region_bytes)
        self.size = self.end + self.guard
        rng = np.random.default_rng(seed)
        self.fill = rng.integers(0, 256, self.size, dtype=np.uint8)
        self.expected = self.fill.copy()
        self.mask = np.zeros(self.size, bool)
        self.operands: dict[str, Operand] = {}
        self._tensor = None

    # ---- layout ----------------------------------------------------------------------------------------------------
    def operand(self, name, offset, n_obj, obj_stride, n_rows, row_stride, width) -> Operand:
        """An output of n_obj x n_rows rows of `width` bytes at the given strides (bytes), `offset` bytes into the
        region.  A flat array of n items of s bytes is (1, 0, n, s, s)."""
        assert self._tensor is None, "lay the arena out before it goes to the device"
        op = Operand(name, int(offset), int(n_obj), int(obj_stride), int(n_rows), int(row_stride), int(width))
        assert name not in self.operands and op.offset >= 0 and self.start + op.offset + op.extent <= self.end, name
        idx = self.start + op.offsets().reshape(-1)
        assert np.unique(idx).size == idx.size and not self.mask[idx].any(), f"{name}: footprint overlaps"
        self.mask[idx] = True
        self.operands[name] = op
        return op

    def expect(self, name, values) -> None:
        """What the call must leave in the operand's footprint: [n_obj][n_rows][width] bytes (an integer array is taken
        as its little-endian bytes)."""
        op = self.operands[name]
        v = np.ascontiguousarray(values)
        v = v.view(np.uint8).reshape(op.n_obj, op.n_rows, op.width)
        self.expected[self.start + op.offsets()] = v

    def seal(self) -> None:
        """Makes every footprint byte's prefill differ from its expected value, so that an unwritten byte can never pass
        by coincidence (the bytes outside the footprint keep the generator's fill)."""
        same = self.mask & (self.fill == self.expected)
        self.fill[same] ^= 0x5A

    # ---- device ----------------------------------------------------------------------------------------------------
    def device(self, device="cuda:0", seal=True):
        """Seals the arena and uploads its prefill: the uint8 device tensor of the whole arena.  seal=False for an
        in-place call, whose output's prefill is its input (a byte it leaves alone is then expected to keep it)."""
        import torch

        if seal:
            self.seal()
        self._tensor = torch.from_numpy(self.fill.copy()).to(device)
        assert self._tensor.data_ptr() % 16 == 0
        return self._tensor

    def ptr(self, name) -> int:
        return self._tensor.data_ptr() + self.start + self.operands[name].offset

    def region(self):
        """The whole region as a flat uint8 torch view."""
        return self._tensor[self.start: self.end]

    def tensor(self, name, shape, dtype=None):
        """A contiguous operand as a torch view of the arena (dtype: torch.int32 / torch.int64 for statuses)."""
        op = self.operands[name]
        t = self._tensor[self.start + op.offset: self.start + op.offset + op.extent]
        if dtype is not None:
            t = t.view(dtype)
        return t.view(*shape)

    def rows(self, name, obj=0):
        """One object's rows as a 2-D strided torch view [n_rows][width]."""
        op = self.operands[name]
        a = self.start + op.offset + obj * op.obj_stride
        return self._tensor.as_strided((op.n_rows, op.width), (op.row_stride, 1), a)

    def after(self) -> np.ndarray:
        import torch

        torch.cuda.synchronize()
        return self._tensor.cpu().numpy()

    def check_device(self) -> None:
        self.check(self.after())

    # ---- the check (pure numpy) ------------------------------------------------------------------------------------
    def locate(self, off: int):
        """(where, operand, object, row, column) of an arena offset: the operand whose row starts closest before it."""
        if off < self.start:
            return "guard before", None, None, None, None
        if off >= self.end:
            return "guard after", None, None, None, None
        best = None
        for op in self.operands.values():
            rel = off - self.start - op.offset
            if rel < 0:
                continue
            o = min(rel // op.obj_stride, op.n_obj - 1) if op.n_obj > 1 else 0
            rel -= o * op.obj_stride
            r = min(rel // op.row_stride, op.n_rows - 1) if op.n_rows > 1 else 0
            c = rel - r * op.row_stride
            if best is None or c < best[4]:
                best = ("region", op.name, int(o), int(r), int(c))
        return best or ("region", None, None, None, None)

    def find(self, after: np.ndarray) -> Finding | None:
        """The first byte of `after` (the arena read back) that is not what the footprint allows, or None."""
        after = np.asarray(after, np.uint8).reshape(-1)
        assert after.size == self.size
        bad = np.flatnonzero(after != self.expected)  # expected = the prefill outside the mask
        if bad.size == 0:
            return None
        off = int(bad[0])
        where, name, o, r, c = self.locate(off)
        return Finding("value" if self.mask[off] else "stray", where, name, o, r, c, off, int(after[off]),
                       int(self.expected[off]))

    def check(self, after: np.ndarray) -> None:
        f = self.find(after)
        if f is not None:
            n = int(np.count_nonzero(np.asarray(after, np.uint8).reshape(-1) != self.expected))
            raise AssertionError(f"{f} ({n} bytes differ)")

    def check_guards(self, after: np.ndarray) -> None:
        """The guards alone, for a buffer whose contents are the library's own (a plan buffer)."""
        after = np.asarray(after, np.uint8).reshape(-1)
        assert after.size == self.size
        for where, lo, hi in (("guard before", 0, self.start), ("guard after", self.end, self.size)):
            bad = np.flatnonzero(after[lo:hi] != self.fill[lo:hi])
            if bad.size:
                off = lo + int(bad[0])
                raise AssertionError(f"stray write outside the footprint at {where} (arena offset {off}, region "
                                     f"[{self.start}, {self.end})): got 0x{after[off]:02X}, want 0x{self.fill[off]:02X}")


def assert_inputs_unchanged(inputs) -> None:
    """inputs: {name: (host copy made before the call, device tensor after it)} -- byte-identical, every one."""
    import torch

    torch.cuda.synchronize()
    for name, (before, t) in inputs.items():
        now = t.cpu().numpy()
        before = np.asarray(before)
        assert now.dtype == before.dtype and now.shape == before.shape, name
        if not np.array_equal(now, before):
            i = int(np.flatnonzero(now.reshape(-1) != before.reshape(-1))[0])
            raise AssertionError(f"input {name} changed by the call: first at flat index {i} "
                                 f"({np.unravel_index(i, before.shape)}): {before.reshape(-1)[i]} -> {now.reshape(-1)[i]}")
