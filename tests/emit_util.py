"""What the tests of the sender's emit share (include/rlnc_hip.h, rlnc_encode_emit): a numpy model of the contract and
the named want patterns.  tests/test_encode_emit_host.py holds the model to a naive per-object loop and every pattern to
its name, so that no test of tests/test_gpu_encode_emit.py passes vacuously.  Plain module: nothing here needs a GPU."""
import numpy as np

from tests.gpu_util import MUL

NONE = -1
MAX_K = 4096
MAX_PER_OBJECT = 4096
MAX_PACKETS = 1 << 20
MAX_OBJECTS = 1 << 20
CHUNK = 1024  # objects per workgroup of the scan launch
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def split_model(want, max_per_object, n):
    """(w, base, g, total, object): w_o = min(max(want_o, 0), max_per_object); base_o = min(sum of the w before o, n);
    g_o = min(w_o, n - base_o); total = min(sum w, n); object int32 [n], NONE from total on.  Vectorised (cumsum,
    repeat), unlike the loop it is tested against."""
    w = np.clip(np.asarray(want, np.int64), 0, max_per_object)
    before = np.concatenate([[0], np.cumsum(w)[:-1]]) if len(w) else np.zeros(0, np.int64)
    base = np.minimum(before, n)
    g = np.minimum(w, n - base)
    total = int(min(w.sum(), n))
    obj = np.full(n, NONE, np.int64)
    obj[:total] = np.repeat(np.arange(len(w)), g)
    assert int(g.sum()) == total
    return w.astype(np.int32), base.astype(np.int32), g.astype(np.int32), total, obj.astype(np.int32)


def naive_split(want, max_per_object, n):
    """The same by the sender's own loop: object after object, packet after packet, while the n packets last."""
    obj, granted, bases = [], [], []
    for o, wo in enumerate(want):
        bases.append(len(obj))  # n once the packets have run out
        wo = min(max(int(wo), 0), max_per_object)
        got = 0
        for _ in range(wo):
            if len(obj) < n:
                obj.append(o)
                got += 1
        granted.append(got)
    total = len(obj)
    return bases, granted, total, obj + [NONE] * (n - total)


def emit_model(src, want, r, max_per_object):
    """(out uint8 [total][k + L], object int32 [n], total, granted int32 [obj]) of an emit of src [obj][k][L] with the
    random bytes r [n][k]: packet i of object o is r[i] || r[i] x src[o], one table lookup per source row over all
    packets at once (gpu_util's multiplication table: independent of the C oracle and of the device kernels)."""
    n, k = r.shape
    _, base, g, total, obj = split_model(want, max_per_object, n)
    out = np.zeros((total, k + src.shape[2]), np.uint8)
    out[:, :k] = r[:total]
    ids = obj[:total]
    for j in range(k):
        out[:, k:] ^= MUL[r[:total, j][:, None], src[ids, j, :]]
    return out, obj, total, g


# ---- named want patterns over `nobj` objects with cap `cap` -----------------------------------------------------------
def _zero_runs(nobj, cap):
    """Zero runs longer than a chunk of 1,024 objects between single nonzero entries (needs nobj > 2 * CHUNK + 2)."""
    w = np.zeros(nobj, np.int64)
    w[0] = cap
    w[CHUNK + 1] = 1
    w[nobj - 1] = cap
    return w


PATTERNS = {
    "all-zero": lambda nobj, cap: np.zeros(nobj, np.int64),
    "all-cap": lambda nobj, cap: np.full(nobj, cap, np.int64),
    "clamped": lambda nobj, cap: np.resize(np.array([-3, cap + 4, INT32_MIN, INT32_MAX, 1, 0, -1, cap]), nobj),
    "zero-runs": _zero_runs,
    "one-takes-all": lambda nobj, cap: np.where(np.arange(nobj) == nobj // 2, cap, 0),
    "last-only": lambda nobj, cap: np.where(np.arange(nobj) == nobj - 1, 1, 0),
}


def pattern(name, nobj, cap):
    w = np.asarray(PATTERNS[name](nobj, cap), np.int64).astype(np.int32)
    assert w.shape == (nobj,)
    w.setflags(write=False)
    return w


def truncation_points(want, max_per_object):
    """The packet capacities at which the split changes character: one below the sum, the sum, one above, every object
    boundary, 1, and inside the first emitting object."""
    w = np.clip(np.asarray(want, np.int64), 0, max_per_object)
    s = int(w.sum())
    ends = np.cumsum(w)
    pts = {1, s - 1, s, s + 1, s + 5} | {int(e) for e in ends} | {int(e) - 1 for e in ends} | {int(e) + 1 for e in ends}
    first = w[np.flatnonzero(w)[0]] if w.any() else 0
    if first > 1:
        pts.add(int(first) // 2)
    return sorted(p for p in pts if 1 <= p <= MAX_PACKETS)
