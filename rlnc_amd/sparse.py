"""Sparse coding vectors on the host (numpy only; importable without a device).

The format of the *_sparse calls (include/rlnc_hip.h, "Sparse coding vectors"), ELL-style with a fixed number w of
entries per row:
    idx  int32 [..., n_out, w]   source-row index of each entry
    val  uint8 [..., n_out, w]   its coefficient
The dense row they stand for is c[j] = XOR of val[t] over all t with idx[t] == j: an entry with val == 0 is padding,
an entry whose index is not in [0, n_in) is dropped, duplicates accumulate by XOR.
"""
from __future__ import annotations

import numpy as np


def to_dense(idx, val, n_in: int) -> np.ndarray:
    """The normative expansion: uint8 [..., n_out, n_in] of idx / val [..., n_out, w]."""
    idx = np.asarray(idx)
    val = np.asarray(val, np.uint8)
    assert idx.shape == val.shape and idx.ndim >= 1 and np.issubdtype(idx.dtype, np.integer)
    out = np.zeros(idx.shape[:-1] + (int(n_in),), np.uint8)
    flat = out.reshape(-1, int(n_in))
    fi = idx.reshape(flat.shape[0], idx.shape[-1]).astype(np.int64)  # (w may be 0)
    fv = val.reshape(fi.shape)
    rows = np.arange(flat.shape[0])
    for t in range(fi.shape[1]):  # entry by entry: duplicates inside a row must not collapse into one write
        ok = (fi[:, t] >= 0) & (fi[:, t] < n_in)
        flat[rows[ok], fi[ok, t]] ^= fv[ok, t]
    return out


def from_dense(coeffs, w: int | None = None):
    """ELL arrays (idx int32, val uint8, both [..., n_out, w]) of a dense matrix [..., n_out, n_in]: each row's
    nonzeros in column order, padded with (0, 0).  w defaults to the largest row count; a row with more than w
    nonzeros raises ValueError."""
    coeffs = np.asarray(coeffs, np.uint8)
    flat = coeffs.reshape(-1, coeffs.shape[-1])
    counts = (flat != 0).sum(axis=1)
    most = int(counts.max()) if counts.size else 0
    if w is None:
        w = most
    if most > w:
        raise ValueError(f"a row has {most} nonzero coefficients, more than w = {w}")
    idx = np.zeros((flat.shape[0], w), np.int32)
    val = np.zeros((flat.shape[0], w), np.uint8)
    for r in range(flat.shape[0]):
        nz = np.flatnonzero(flat[r])
        idx[r, : nz.size] = nz
        val[r, : nz.size] = flat[r, nz]
    shape = coeffs.shape[:-1] + (w,)
    return idx.reshape(shape), val.reshape(shape)


def draw(rng, n: int, k: int, w: int):
    """n sparse coding vectors over k sources: min(w, k) distinct indices each with values in 1..255, padded to w
    entries with (0, 0).  Returns (idx int32 [n][w], val uint8 [n][w])."""
    m = min(int(w), int(k))
    idx = np.zeros((n, w), np.int32)
    val = np.zeros((n, w), np.uint8)
    for i in range(n):
        idx[i, :m] = rng.choice(k, size=m, replace=False)
        val[i, :m] = rng.integers(1, 256, m, dtype=np.uint8)
    return idx, val
