"""What the tests of a decode stream's accept share (include/rlnc_hip.h, rlnc_decode_stream_accept): a numpy model of
the contract and the named id patterns.  tests/test_decode_stream_accept_host.py holds every pattern to its name, so
that no test of tests/test_gpu_decode_stream_accept.py passes vacuously.  Plain module: nothing here needs a GPU."""
import numpy as np

NO_ROOM, NO_OBJECT, FINISHED, ABSENT = -1, -2, -3, -4
MAX_ARRIVALS = 1 << 20
CHUNK = 1024  # arrivals per workgroup of the rank launch
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def taken(n, count):
    """n' = min(max(count, 0), n); count None: n."""
    return n if count is None else min(max(int(count), 0), n)


def accept_model(objects, avail, m, num_objects, count=None, finished=None):
    """(slot int32 [n], avail int32 [obj], refused int32 [obj]) after an accept of the ids `objects` on `avail`;
    finished: a bool mask [obj] of the objects whose rank is k, or None for a call without a state.  A stable ranking
    per object (argsort, kind="stable"), then the clamps, the overflow, the finished filter and the count."""
    objects = np.asarray(objects, np.int64)
    avail = np.asarray(avail, np.int64)
    n, npr = len(objects), taken(len(objects), count)
    fin = np.zeros(num_objects, bool) if finished is None else np.asarray(finished, bool)
    slot = np.full(n, ABSENT, np.int64)
    ids = objects[:npr]
    valid = (ids >= 0) & (ids < num_objects)
    slot[:npr][~valid] = NO_OBJECT
    idx = np.flatnonzero(valid)
    order = idx[np.argsort(ids[idx], kind="stable")]  # grouped by object, in arrival order inside a group
    sid = ids[order]
    cnt = np.bincount(sid, minlength=num_objects)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    j = np.arange(len(order)) - start[sid]
    a = np.clip(avail, 0, m)
    s = a[sid] + j
    s = np.where(s < m, s, NO_ROOM)
    slot[order] = np.where(fin[sid], FINISHED, s)
    new_avail = np.where(fin, avail, np.minimum(a + cnt, m))
    refused = np.where(fin, 0, np.maximum(a + cnt - m, 0))
    return slot.astype(np.int32), new_avail.astype(np.int32), refused.astype(np.int32)


def place(pieces, arrivals, objects, slot):
    """pieces [obj][m][k + L] with every placed arrival copied to its slot (a new array)."""
    out = np.array(pieces, copy=True)
    placed = np.flatnonzero(np.asarray(slot) >= 0)
    out[np.asarray(objects)[placed], np.asarray(slot)[placed]] = np.asarray(arrivals)[placed]
    return out


def host_loop(pieces, arrivals, objects, filled, m):
    """INTEGRATION.md's receive loop on numpy arrays: one copy per arrival into pieces[o][filled[o]], arrivals beyond m
    dropped.  (pieces, filled) afterwards, both new."""
    out, filled = np.array(pieces, copy=True), list(filled)
    for piece, o in zip(arrivals, objects):
        if filled[o] < m:
            out[o, filled[o]] = piece
            filled[o] += 1
    return out, filled


# ---- order: k + L = 6, m = 8,192, 3 objects --------------------------------------------------------------------------
ORDER_SHAPE = (2, 4, 8192, 3)  # k, L, m, objects
ORDER_N = 3000


def _skewed(rng):
    return rng.choice(3, ORDER_N, p=[0.9, 0.08, 0.02])


def _straddle(rng):
    """The only equal valid ids lie on both sides of a chunk boundary: 0 at 1,023 / 1,024 and 1 at 2,047 / 2,048; object
    2 comes once; every other id is beyond the objects (distinct, so that nothing else could be ranked with another)."""
    ids = 3 + np.arange(2 * CHUNK + 100)
    ids[[CHUNK - 1, CHUNK]] = 0
    ids[[2 * CHUNK - 1, 2 * CHUNK]] = 1
    ids[5] = 2
    return ids


PATTERNS = {
    "one-1023": lambda rng: np.zeros(1023, int),
    "one-1024": lambda rng: np.ones(1024, int),
    "one-1025": lambda rng: np.full(1025, 2),
    "one-3000": lambda rng: np.zeros(3000, int),
    "one-9000": lambda rng: np.ones(9000, int),  # above m
    "round-robin": lambda rng: np.arange(ORDER_N) % 3,
    "sorted": lambda rng: np.sort(rng.integers(0, 3, ORDER_N)),
    "reverse-sorted": lambda rng: np.sort(rng.integers(0, 3, ORDER_N))[::-1].copy(),
    "skewed": _skewed,
    "straddle": _straddle,
    "single": lambda rng: np.array([1]),
}


def pattern(name):
    ids = np.asarray(PATTERNS[name](np.random.default_rng(sorted(PATTERNS).index(name))), np.int32)
    ids.setflags(write=False)
    return ids


# ---- piece widths: 9 objects, m = 7, n = 40 --------------------------------------------------------------------------
WIDTHS = [2, 15, 17, 4095, 4096, 4097, 8191, 12305]
WIDTH_OBJECTS, WIDTH_M, WIDTH_N = 9, 7, 40
WIDTH_AVAIL = (3, 4, 2, 5, 3, 4, 6, 7, 1)


def width_ids():
    ids = np.random.default_rng(77).integers(0, WIDTH_OBJECTS, WIDTH_N).astype(np.int32)
    ids.setflags(write=False)
    return ids


# ---- every code in one call: 5 objects of m = 6 ----------------------------------------------------------------------
def codes_case():
    """(ids, avail, m, objects, count, finished): one call in which every negative code occurs, an object overflows, an
    object has no arrival, and the avail inputs are -5, 0, m - 1, m and m + 3."""
    m, nobj = 6, 5
    avail = np.array([-5, 0, m - 1, m, m + 3], np.int32)
    ids = np.array([1, 0, -1, 2, 2, nobj, 3, 1, INT32_MIN, 2, 0, INT32_MAX, 1, 3, 0, 1, 2, 0], np.int32)
    finished = np.array([False, True, False, False, False])
    return ids, avail, m, nobj, len(ids) - 3, finished
