"""Structured families of coding vectors, and what the reference's elimination does on each.

Random vectors leave the clean state of the rank-mode-0 elimination (rows 0 .. c - 1 with M[i][i] = 1 and column i zero
in every other one of them) rarely and briefly.  The families below hold it, leave it for the whole matrix, or go in and
out of it many times, by construction; they are also what real traffic looks like (systematic, banded, GF(2), relayed in
any order).  reference_trace / profile say, from the reference oracle alone, which state each one reaches, so that the
tests can assert that they reach it.  Plain module: no GPU, no library."""
import numpy as np

from tests.gpu_util import np_matmul
from tests.true_rank import FIXTURE, FIXTURE_K, OK

NAMES = ["identity", "reversed", "shift", "perm", "upper", "upper_rev", "lower", "lower_rev", "band", "gf2", "halves",
         "highspan", "fixture_blocks", "lowrank", "dupzero"]
BAND = 4  # nonzero columns of a `band` row


def _nonzero(rng, shape):
    return rng.integers(1, 256, shape, dtype=np.uint8)


def _scaled_units(rng, k, cols):
    out = np.zeros((k, k), np.uint8)
    out[np.arange(k), cols] = _nonzero(rng, k)
    return out


def _rows(name, k, rng):
    """The k x k family itself (rows 0 .. k - 1 of family())."""
    eye = np.eye(k, dtype=np.uint8)
    h = k // 2
    if name == "identity":
        return eye
    if name == "reversed":
        return eye[::-1].copy()
    if name == "shift":
        return _scaled_units(rng, k, (np.arange(k) + 1) % k)
    if name == "perm":
        return _scaled_units(rng, k, rng.permutation(k))
    d = _nonzero(rng, (k, k))
    if name in ("upper", "upper_rev"):
        u = np.triu(d)
        return u if name == "upper" else u[::-1].copy()
    if name in ("lower", "lower_rev"):
        lo = np.tril(d)
        return lo if name == "lower" else lo[::-1].copy()
    if name == "band":
        b = np.zeros((k, k), np.uint8)
        for i in range(k):
            b[i, i:i + BAND] = d[i, i:i + BAND]
        return b[rng.permutation(k)]
    if name == "gf2":
        return rng.integers(0, 2, (k, k), dtype=np.uint8)
    if name == "halves":
        d[:h, :h] = 0
        d[h:, h:] = 0
        return d
    if name == "highspan":  # rows 0 .. h + 3 span at most the h high columns
        d[:h + 4, :k - h] = 0
        return d
    if name == "fixture_blocks":
        nb = k // FIXTURE_K
        for b in range(nb):
            d[4 * b:4 * b + 4] = 0
            d[4 * b:4 * b + 4, FIXTURE_K * b:FIXTURE_K * (b + 1)] = FIXTURE
        return d
    if name == "lowrank":
        return np_matmul(_nonzero(rng, (k, max(h, 1))), d[:max(h, 1)])
    if name == "dupzero":  # 0, v0, v0, v1, v1, ...
        out = np.zeros((k, k), np.uint8)
        out[1:] = d[np.arange(k - 1) // 2]
        return out
    raise KeyError(name)


def family(name, k, m, rng):
    """[m][k] uint8 coding vectors: rows 0 .. min(m, k) - 1 are the family, rows from k on dense random."""
    n = min(m, k)
    return np.concatenate([_rows(name, k, rng)[:n], rng.integers(0, 256, (m - n, k), dtype=np.uint8)])


# the seeds of vectors() at which a seeded family meets its reach condition where seed 0 does not: perm and band are
# clean again exactly after piece k - 1, gf2 returns to clean three times without more than 8 dirty rows
# (tests/test_coding_families_host.py, tests/test_gpu_coding_families.py)
SEEDS = {("perm", 8, 12): 1, ("band", 8, 12): 2, ("gf2", 128, 130): 1, ("gf2", 200, 260): 1}


def vectors(name, k, m, seed=None):
    """family() under the generator of (name, k, m, seed); seed None: the shape's kept seed."""
    if seed is None:
        seed = SEEDS.get((name, k, m), 0)
    return family(name, k, m, np.random.default_rng([NAMES.index(name), k, m, seed]))


def clean_prefix(M, k):
    """The largest c with M[:c, :c] the identity: rows 0 .. c - 1 have M[i][i] = 1 and column i zero in the others."""
    n = min(M.shape[0], k)
    c = 0
    while c < n and M[c, c] == 1 and not M[c, :c].any() and not M[:c, c].any():
        c += 1
    return c


def reference_trace(k, pieces):
    """OracleDecoder over pieces [m][k + L] (or bare coding vectors [m][k]: one zero payload byte is added), piece by
    piece.  Returns (statuses, rows, clean): after piece p the matrix has rows[p] rows, the first clean[p] of them the
    clean prefix."""
    from oracle.oracle import OracleDecoder

    pieces = np.asarray(pieces, np.uint8)
    if pieces.shape[1] == k:
        pieces = np.concatenate([pieces, np.zeros((pieces.shape[0], 1), np.uint8)], axis=1)
    od = OracleDecoder(pieces.shape[1] - k, k)
    st, rows, clean = [], [], []
    for p in pieces:
        st.append(od.decode(np.ascontiguousarray(p)))
        M = od.matrix()
        rows.append(M.shape[0])
        clean.append(clean_prefix(M, k))
    return st, rows, clean


def profile(trace, model):
    """trace: reference_trace's result; model: true_rank_model's, on the same vectors."""
    st, rows, clean = trace
    dirty = [r - c for r, c in zip(rows, clean)]
    return {
        "dirty_pieces": sum(1 for x in dirty if x),
        "max_dirty_rows": max(dirty, default=0),
        "reclean": [p for p in range(1, len(dirty)) if dirty[p - 1] and not dirty[p]],
        "useful": ([0] + [r for r, s in zip(rows, st) if s == OK])[-1],  # Decoder::get_useful_piece_count
        "true_rank": model[1],
        "differ": [p for p, (a, b) in enumerate(zip(st, model[0])) if a != b],
    }
