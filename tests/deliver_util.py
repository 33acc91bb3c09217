"""The batches the delivery tests run on (include/rlnc_hip.h, rlnc_decode_stream_deliver): per shape (k, m, L), nine
objects by name, each with a real payload -- the oracle's padded image of a seeded byte string whose length differs per
object -- and pieces [co | co x src] computed with oracle/np_oracle.py's field.  tests/test_decode_stream_deliver_host.py
asserts with the true-rank model that every object has the rank, done and statuses its name claims.  Numpy only: no GPU.

  exact      k independent dense vectors in slots 0..k-1; done = k
  padded     a zero vector, a duplicate and a multiple interleaved among the useful ones (as many of the three as m - k
             and k leave room for): rank k is reached at done > k, and T has zero columns between nonzero ones
  over       rank k is reached at slot k - 1 < done: the later slots are ReceivedAllPieces
  short      rank k - 1
  deficient  all m slots pushed inside a (k - 1)-dimensional span: done = m, rank < k
  empty      nothing pushed
  badmarker  rank k over a payload whose last nonzero byte is not 0x81
  zeros      rank k over an all-zero payload
  sparse     density-2 vectors of full rank
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import np_oracle as npo
from tests.gpu_util import np_matmul
from tests.true_rank import MUL, NOT_USEFUL, OK, RECEIVED_ALL

# (k, m, L): the smallest shapes that reach every path of the delivery
#   (1, 3, 4)         tail kernel only, one row
#   (3, 5, 4099)      k < 4 across a column block
#   (4, 1100, 4096)   1-wave program at its four-row minimum, n_in up to 1,100
#   (5, 9, 4096)      1-wave program, exactly one block, no tail launch
#   (16, 20, 4099)    2-wave program, one block plus 3 bytes
#   (24, 40, 8209)    4-wave shared program, two blocks plus 17 bytes
#   (40, 48, 4096)    8-wave program, one partly filled row tile
#   (70, 80, 4100)    8-wave program, two row tiles, the second with 6 rows
#   (300, 330, 4099)  five row tiles; the workspace push form
SHAPES = [(1, 3, 4), (3, 5, 4099), (4, 1100, 4096), (5, 9, 4096), (16, 20, 4099), (24, 40, 8209), (40, 48, 4096),
          (70, 80, 4100), (300, 330, 4099)]
# the shape of the refusal test: one that no other test initialises a stream for
REFUSAL_SHAPE = (12, 22, 4099)
NAMES = ["exact", "padded", "over", "short", "deficient", "empty", "badmarker", "zeros", "sparse"]
FULL = ("exact", "padded", "over", "badmarker", "zeros", "sparse")  # the objects of rank k
NOT_ALL, BAD_FORMAT = 10, 11  # NotAllPiecesReceivedYet, InvalidDecodedDataFormat


@dataclass(frozen=True)
class Batch:
    k: int
    m: int
    L: int
    co: np.ndarray       # [9][m][k] coding vectors of every slot (slots at or beyond done: never pushed)
    done: tuple          # slots pushed, per object
    rank: tuple          # the rank the name claims after them
    statuses: tuple      # ... and the piece statuses of the pushed slots
    src: np.ndarray      # [9][k][L] source rows
    data_len: tuple      # the payload's byte length (what a valid marker answers)
    pieces: np.ndarray   # [9][m][k + L]; the slots never pushed hold seeded bytes, not pieces
    status: tuple        # the object status a delivery answers
    length: tuple        # ... and the length


def independent(rng, k):
    """k independent dense vectors: a unit lower times a unit upper triangular matrix with nonzero fill."""
    lo = np.tril(rng.integers(1, 256, (k, k), dtype=np.uint8), -1) | np.eye(k, dtype=np.uint8)
    up = np.triu(rng.integers(1, 256, (k, k), dtype=np.uint8), 1) | np.eye(k, dtype=np.uint8)
    return np_matmul(lo, up)


def density2(rng, k):
    """k vectors of (at most) two nonzeros and full rank: a_i e_i + b_i e_(i+1 mod k), whose determinant is the product
    of the a's plus the product of the b's."""
    if k == 1:
        return rng.integers(1, 256, (1, 1), dtype=np.uint8)
    a, b = rng.integers(1, 256, k, dtype=np.uint8), rng.integers(1, 256, k, dtype=np.uint8)
    prod = lambda v: functools.reduce(lambda x, y: int(MUL[x][y]), [int(t) for t in v])  # noqa: E731
    if prod(a) == prod(b):
        b[0] = b[0] % 255 + 1  # another nonzero value: the product changes
    v = np.zeros((k, k), np.uint8)
    for i in range(k):
        v[i, i], v[i, (i + 1) % k] = a[i], b[i]
    return v[rng.permutation(k)]


def payload(rng, k, L, o, kind):
    """(source rows [k][L], payload length)."""
    n = k * L - 1 - (o % k)
    src = npo.pad(rng.integers(0, 256, n, dtype=np.uint8), k)
    assert src.shape == (k, L)
    if kind == "badmarker":
        src.reshape(-1)[n] = 0x80
    if kind == "zeros":
        src[:] = 0
    return src, n


@functools.lru_cache(maxsize=None)
def batch(k, m, L):
    rng = np.random.default_rng(9000 * k + 10 * m + L % 7)
    co = rng.integers(1, 256, (len(NAMES), m, k), dtype=np.uint8)  # whatever lies beyond done is never pushed
    done, rank, sts, srcs, lens, ost, olen = [], [], [], [], [], [], []
    extra = min(2, m - k)
    for o, name in enumerate(NAMES):
        u = density2(rng, k) if name == "sparse" else independent(rng, k)
        if name in ("exact", "badmarker", "zeros", "sparse"):
            seq, st = list(u), [OK] * k
        elif name == "padded":
            nj = min(3, m - k)
            assert nj >= 1
            seq, st = [np.zeros(k, np.uint8), u[0]], [NOT_USEFUL, OK]
            if k >= 2 and nj >= 2:
                seq.append(u[0].copy()), st.append(NOT_USEFUL)
            if k == 2 and nj >= 3:
                seq.append(MUL[0x1D][u[0]]), st.append(NOT_USEFUL)
            for i in range(1, k):
                seq.append(u[i]), st.append(OK)
                if i == 1 and k >= 3 and nj >= 3:
                    seq.append(MUL[0x1D][u[0]]), st.append(NOT_USEFUL)
        elif name == "over":
            seq, st = list(u) + list(co[o, k: k + extra]), [OK] * k + [RECEIVED_ALL] * extra
        elif name == "short":
            seq, st = list(u[: k - 1]), [OK] * (k - 1)
        elif name == "deficient":
            if k == 1:
                seq = [np.zeros(1, np.uint8)] * m
            else:
                seq = list(np_matmul(rng.integers(0, 256, (m, k - 1), dtype=np.uint8), u[: k - 1]))
            st = None  # by the model (the host test): rank < k is what the name claims
        else:
            seq, st = [], []
        assert len(seq) <= m, (name, k, m)
        if seq:
            co[o, : len(seq)] = np.stack(seq)
        full = name in FULL
        src, n = payload(rng, k, L, o, name)
        done.append(len(seq))
        rank.append(k if full else None if name == "deficient" else len(seq))
        sts.append(None if st is None else tuple(st))
        srcs.append(src)
        lens.append(n)
        valid = full and name not in ("badmarker", "zeros")
        ost.append(0 if valid else BAD_FORMAT if full else NOT_ALL)
        olen.append(n if valid else 0)
    src = np.stack(srcs)
    pieces = rng.integers(0, 256, (len(NAMES), m, k + L), dtype=np.uint8)
    for o in range(len(NAMES)):
        d = done[o]
        pieces[o, :d, :k] = co[o, :d]
        if d:
            # density-2 vectors: the product at the cost of the nonzeros
            pieces[o, :d, k:] = (npo.matmul if NAMES[o] == "sparse" else np_matmul)(co[o, :d], src[o])
    for a in (co, src, pieces):
        a.setflags(write=False)
    return Batch(k, m, L, co, tuple(done), tuple(rank), tuple(sts), src, tuple(lens), pieces, tuple(ost), tuple(olen))
