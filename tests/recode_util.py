"""The batches the stream-recode tests run on (include/rlnc_hip.h, rlnc_decode_stream_recode): per shape (k, m, L,
count), nine objects by name, each with a real payload (tests/deliver_util.py's: the oracle's padded image of a seeded
byte string) and pieces [co | co x src] computed with oracle/np_oracle.py's field.  The expected output of object o is
np_matmul(r[o][:, :rank], pieces[o][u]) over the full pieces, u the useful slots in arrival order.
tests/test_decode_stream_recode_host.py asserts with the true-rank model that every object has the rank, done and Ok list
its name claims.  Numpy only: no GPU.

  exact       k independent dense vectors in slots 0..k-1; done = k
  padded      a zero vector, a duplicate and a multiple interleaved among the useful ones (as many of the three as m - k
              and k leave room for): done > rank = k, u has gaps
  chain       slot 0 a zero vector and every later pushed slot useful: u_j = j + 1
  over        rank k is reached at slot k - 1 < done: the later slots are ReceivedAllPieces and must be left out
  short       rank k - 1
  deficient   all m slots pushed inside a (k - 1)-dimensional span: done = m, rank = k - 1, u by the model
  empty       nothing pushed
  zeros-only  zero vectors pushed: done > 0, rank 0
  sparse      density-2 vectors of full rank
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import np_oracle as npo
from tests.deliver_util import density2, independent, payload
from tests.gpu_util import np_matmul
from tests.stream_util import model_of
from tests.true_rank import MUL, NOT_USEFUL, OK, RECEIVED_ALL

# (k, m, L, count): the smallest shapes that reach every path of the recode; the product's width is k + L
#   (1, 3, 4, 1)         tail kernel only, one row
#   (3, 5, 4099, 3)      count < 4 across a column block
#   (5, 9, 4091, 4)      width exactly 4,096: the 1-wave program at its four-row minimum, no tail launch
#   (4, 1100, 4096, 8)   n_in up to 1,100 (deficient: done = m), the status scan beyond one pass of 256 threads
#   (16, 20, 4099, 16)   2-wave program, header and data straddling the first block
#   (24, 67, 8209, 24)   4-wave shared program, m not a multiple of 4
#   (40, 48, 4096, 40)   8-wave program, one partly filled tile
#   (16, 24, 4100, 70)   count > k: two row tiles of the 8-wave program, the second with 6 rows
#   (300, 330, 4099, 8)  the workspace push form, an Ok list longer than 256
#   (4, 8192, 60, 4)     the most slots a stream takes
SHAPES = [(1, 3, 4, 1), (3, 5, 4099, 3), (5, 9, 4091, 4), (4, 1100, 4096, 8), (16, 20, 4099, 16), (24, 67, 8209, 24),
          (40, 48, 4096, 40), (16, 24, 4100, 70), (300, 330, 4099, 8), (4, 8192, 60, 4)]
# the shape of the refusal test: one that no other test initialises a stream for
REFUSAL_SHAPE = (12, 23, 4099, 5)
NAMES = ["exact", "padded", "chain", "over", "short", "deficient", "empty", "zeros-only", "sparse"]
FULL = ("exact", "padded", "over", "sparse")  # the objects of rank k
NOT_ENOUGH = 6  # NotEnoughPiecesToRecode


@dataclass(frozen=True)
class Batch:
    k: int
    m: int
    L: int
    count: int
    co: np.ndarray       # [9][m][k] coding vectors of every slot (slots at or beyond done: never pushed)
    done: tuple          # slots pushed, per object
    rank: tuple          # the rank after them
    useful: tuple        # the slots below done whose status is Ok, in order (by construction; deficient: by the model)
    statuses: tuple      # the piece statuses of the pushed slots the name claims (None: deficient, left to the model)
    src: np.ndarray      # [9][k][L] source rows
    data_len: tuple      # the payload's byte length
    pieces: np.ndarray   # [9][m][k + L]; the slots never pushed hold seeded bytes, not pieces
    r: np.ndarray        # [9][count][k] the random bytes of a recode; those from the rank on must be ignored
    status: tuple        # the status a recode answers
    expected: tuple      # [count][k + L] per object, None for rank 0


def expected_of(b, o, r):
    """What a recode of object o with the random bytes r [count][k] writes: None for rank 0."""
    if b.rank[o] == 0:
        return None
    return np_matmul(r[:, : b.rank[o]], b.pieces[o][list(b.useful[o])])


@functools.lru_cache(maxsize=None)
def batch(k, m, L, count):
    rng = np.random.default_rng(11000 * k + 13 * m + L % 7 + 100003 * count)
    co = rng.integers(1, 256, (len(NAMES), m, k), dtype=np.uint8)  # whatever lies beyond done is never pushed
    done, rank, useful, sts, srcs, lens = [], [], [], [], [], []
    extra = min(2, m - k)
    for o, name in enumerate(NAMES):
        u = density2(rng, k) if name == "sparse" else independent(rng, k)
        if name in ("exact", "sparse"):
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
        elif name == "chain":
            n = min(k, m - 1)
            seq, st = [np.zeros(k, np.uint8)] + list(u[:n]), [NOT_USEFUL] + [OK] * n
        elif name == "over":
            seq, st = list(u) + list(co[o, k: k + extra]), [OK] * k + [RECEIVED_ALL] * extra
        elif name == "short":
            seq, st = list(u[: k - 1]), [OK] * (k - 1)
        elif name == "deficient":
            if k == 1:
                seq = [np.zeros(1, np.uint8)] * m
            else:
                seq = list(np_matmul(rng.integers(0, 256, (m, k - 1), dtype=np.uint8), u[: k - 1]))
            st = None  # by the model
        elif name == "zeros-only":
            seq, st = [np.zeros(k, np.uint8)] * min(3, m), [NOT_USEFUL] * min(3, m)
        else:
            seq, st = [], []
        assert len(seq) <= m, (name, k, m)
        if seq:
            co[o, : len(seq)] = np.stack(seq)
        if st is None:
            st_model = model_of(k, co[o, : len(seq)])[0]
            ok = tuple(t for t, s in enumerate(st_model) if s == OK)
        else:
            ok = tuple(t for t, s in enumerate(st) if s == OK)
        src, n = payload(rng, k, L, o, name)
        done.append(len(seq))
        rank.append(len(ok))
        useful.append(ok)
        sts.append(None if st is None else tuple(st))
        srcs.append(src)
        lens.append(n)
    src = np.stack(srcs)
    pieces = rng.integers(0, 256, (len(NAMES), m, k + L), dtype=np.uint8)
    for o in range(len(NAMES)):
        d = done[o]
        pieces[o, :d, :k] = co[o, :d]
        if d:
            # density-2 vectors: the product at the cost of the nonzeros
            pieces[o, :d, k:] = (npo.matmul if NAMES[o] == "sparse" else np_matmul)(co[o, :d], src[o])
    r = rng.integers(1, 256, (len(NAMES), count, k), dtype=np.uint8)
    if count * k > 1:  # zeros among the coefficients too
        o_, i_, j_ = np.indices(r.shape)
        r[(o_ + i_ + 2 * j_) % 5 == 4] = 0
    for a in (co, src, pieces, r):
        a.setflags(write=False)
    b = Batch(k, m, L, count, co, tuple(done), tuple(rank), tuple(useful), tuple(sts), src, tuple(lens), pieces, r,
              tuple(0 if x else NOT_ENOUGH for x in rank), ())
    exp = tuple(expected_of(b, o, r[o]) for o in range(len(NAMES)))
    for e in exp:
        if e is not None:
            e.setflags(write=False)
    return Batch(k, m, L, count, co, b.done, b.rank, b.useful, b.statuses, src, b.data_len, pieces, r, b.status, exp)
