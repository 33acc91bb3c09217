"""What the decode-stream tests share (include/rlnc_hip.h, "Decode streams"): the rank-mode-1 context, the device
buffers, the model of each object's prefix and the snapshot check, the host view of a state buffer, and the numpy model
of a compaction with the batches it is tested on.  Plain module: nothing here needs a GPU until it is called."""
import functools

import numpy as np

from tests import limit_shapes as ls
from tests.gpu_util import dev, host
from tests.limit_shapes import large_layout
from tests.true_rank import MUL, OK, sparse_vectors, true_rank_model

PENDING = -1


def true_rank_context():
    """A context on device 0 in rank mode 1: what the ctx1 fixtures return."""
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    assert c.rank_mode == 0
    c.set_rank_mode(1)
    assert c.rank_mode == 1
    return c


def i32(n, fill=-7):
    import torch

    return torch.full(n if isinstance(n, tuple) else (n,), fill, dtype=torch.int32, device="cuda:0")


def pieces_of(co, L=4, seed=0):
    """co [nobj][m][k] -> device pieces [nobj][m][k + L] with random data bytes (the elimination reads none)."""
    nobj, m, k = co.shape
    p = np.random.default_rng(seed).integers(0, 256, (nobj, m, k + L), dtype=np.uint8)
    p[:, :, :k] = co
    return dev(p)


class Prefixes:
    """true_rank_model of object o's first n slots, computed once per (o, n)."""

    def __init__(self, k, co):
        self.k, self.co, self.memo = k, co, {}

    def __call__(self, o, n):
        if (o, n) not in self.memo:
            self.memo[(o, n)] = (true_rank_model(self.k, self.co[o, :n]) if n else
                                 ([], 0, np.zeros((self.k, 0), np.uint8), None))
        return self.memo[(o, n)]


def advance(done, avail, m, max_new):
    return [min(max(a, d), m, d + (m if max_new is None else max_new)) for d, a in zip(done, avail)]


def check_snapshot(stream, model, done, tag):
    import torch

    nobj, k, m = stream.num_objects, stream.k, stream.m
    T = torch.full((nobj, k, m), 0xAA, dtype=torch.uint8, device="cuda:0")
    ps, rk = i32((nobj, m)), i32(nobj)
    stream.snapshot(T, ps, rk)
    T, ps, rk = host(T), host(ps), host(rk)
    for o in range(nobj):
        st, rank, Tm, _ = model(o, done[o])
        assert list(ps[o, :done[o]]) == st, (tag, o)
        assert (ps[o, done[o]:] == PENDING).all(), (tag, o)
        assert rk[o] == rank, (tag, o, rk[o], rank)
        assert np.array_equal(T[o][:, :done[o]], Tm), (tag, o)
        assert not T[o][:, done[o]:].any(), (tag, o)
    return ps, rk


def raw(ctx, fn, *args):
    return getattr(ctx.lib, fn)(ctx.h, *args)


def state_words(image, k, m, nobj):
    """A state buffer's host image (uint8) as uint32 [nobj][total]."""
    total = large_layout(k, m)["total"]
    return np.ascontiguousarray(image[: nobj * total * 4]).view(np.uint32).reshape(nobj, total)


def live_state(image, k, m, nobj):
    """What a later call reads of each object: (rank, done, piv[0..rank), St[0..done), R[0..rank)[D])."""
    lay = large_layout(k, m)
    out = []
    for w in state_words(image, k, m, nobj):
        rank, done = int(w[0]), int(w[2])
        assert 0 <= rank <= k and 0 <= done <= m
        out.append((rank, done, w[lay["piv"]: lay["piv"] + rank].tobytes(), w[lay["st"]: lay["st"] + done].tobytes(),
                    w[lay["r"]: lay["r"] + rank * lay["D"]].tobytes()))
    return out


# ---- compaction: the model and the batches (tests/test_decode_stream_compact_host.py asserts what they hold) ---------
# (5, 7) odd kd, m no multiple of 4; (16, 20) the form the default picks is the LDS one; (24, 67) B = 32, m no multiple
# of 4; (4, 1100) rows wider than 256 dwords; (300, 330) a scan and a list beyond one pass of 256 threads; (4, 8192) the
# most slots a stream takes: 32 statuses per thread of the scan, an e part of 2,048 dwords, slot indices up to 8,190
SHAPES = [(5, 7), (16, 20), (24, 67), (4, 1100), (300, 330), (4, 8192)]
NAMES = ["mixed", "chain", "late", "idle", "empty", "full", "sparse", "planted", "dense"]


def model_of(k, vectors):
    """true_rank_model, and the empty prefix."""
    if len(vectors) == 0:
        return [], 0, np.zeros((k, 0), np.uint8), None
    return true_rank_model(k, vectors)


def compact_model(k, co_prefix):
    """What rlnc_decode_stream_compact does with an object whose pushed slots hold the vectors co_prefix: (u, r, T, st)
    -- the kept slots u_0 < ... < u_{r-1} (the prefix's Ok slots), r = rank, T [k][r] the prefix's T with its columns
    gathered by u, and the prefix's statuses."""
    st, rank, T, _ = model_of(k, co_prefix)
    u = [t for t, s in enumerate(st) if s == OK]
    assert len(u) == rank
    return u, rank, np.ascontiguousarray(T[:, u]), st


@functools.lru_cache(maxsize=None)
def cases(k, m):
    """The batch of a shape: (co uint8 [9][m][k], done [9]) -- each object's coding vectors and how many of its slots
    are pushed before the compaction (a strict prefix: done < m), in the order of NAMES:
      mixed    dense with a zero piece, a duplicate and a multiple among the first slots
      chain    slot 0 zero and every later pushed slot useful: u_j = j + 1 throughout, the longest overwrite chain
      late     the first m - k slots zero, the others dense
      idle     independent vectors only: done == rank > 0
      empty    done == 0
      full     dense: rank k, then ReceivedAllPieces slots below done
      sparse   sparse_vectors at density 2
      planted  limit_shapes.planted: duplicates, multiples and sums of earlier pieces
      dense    dense random, pushed up to m - 2"""
    rng = np.random.default_rng(7000 * k + m)
    dense = lambda: rng.integers(1, 256, (m, k), dtype=np.uint8)  # noqa: E731
    mixed = dense()
    mixed[1] = 0
    mixed[3] = mixed[2]
    mixed[4] = MUL[0x1D][mixed[0]]
    chain = dense()
    chain[0] = 0
    late = dense()
    late[: m - k] = 0
    co = np.stack([mixed, chain, late, dense(), dense(), dense(), sparse_vectors(rng, k, m, 2), ls.planted(rng, k, m),
                   dense()])
    done = [m - 1, min(m - 1, k + 1), m - 1, max(1, k - 2), 0, m - 1, m - 1, m - 1, m - 2]
    co.setflags(write=False)
    return co, tuple(done)


@functools.lru_cache(maxsize=None)
def prefix_models(k, m):
    """compact_model of every object of cases(k, m), computed once."""
    co, done = cases(k, m)
    return tuple(compact_model(k, co[o, :done[o]]) for o in range(co.shape[0]))


@functools.lru_cache(maxsize=None)
def kept_models(k, m):
    """true_rank_model of every object's kept vectors alone, computed once."""
    co, _ = cases(k, m)
    return tuple(model_of(k, co[o][u]) for o, (u, _, _, _) in enumerate(prefix_models(k, m)))
