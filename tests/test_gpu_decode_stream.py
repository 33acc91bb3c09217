"""GPU: decode streams (include/rlnc_hip.h, "Decode streams"; rlnc_amd.batch.DecodeStream) -- the true-rank decode of
rank_large.hip kept on the device between calls and pushed forward per object -- against the numpy model of
tests/true_rank.py run on each object's own prefix.  All comparisons are exact.

After every push a snapshot must be the model of the slots pushed so far: statuses (pending beyond them), rank, T (zero
columns beyond them), and the rank / answered arrays of the push itself.  The shapes are the smallest at which the
kernels can go wrong; each schedule says which cases its rounds are there for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests import limit_shapes as ls
from tests.footprint import Arena, assert_inputs_unchanged
from tests.gpu_util import dev, host
from tests.limit_shapes import block_cases
from tests.stream_util import (PENDING, Prefixes, advance, check_snapshot, i32, pieces_of, raw,
                               true_rank_context)
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL, sparse_vectors, true_rank_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_ALL_YET, INVALID = 10, 100
LARGE = 8
M28 = ls._M32 + 4  # B = 28


@pytest.fixture(scope="module")
def ctx1():
    return true_rank_context()


def run_schedule(ctx, k, co, rounds):
    """rounds: [(avail per object, max_new or None)].  After every push: rank / answered of the push and a snapshot
    against the model of each object's prefix.  avail is overwritten right after the push is enqueued."""
    import torch

    from rlnc_amd import batch

    nobj, m, _ = co.shape
    pieces = pieces_of(co, seed=k + m)
    model = Prefixes(k, co)
    stream = batch.DecodeStream(k, m, nobj, ctx)
    done = [0] * nobj
    history = [list(done)]
    check_snapshot(stream, model, done, "init")
    for r, (avail, max_new) in enumerate(rounds):
        av = torch.tensor(avail, dtype=torch.int32, device="cuda:0")
        rank, answered = i32(nobj), i32(nobj)
        stream.push(pieces, av, max_new, rank, answered)
        av.fill_(m + 12345)  # the push latched its targets: nothing reads avail any more
        done = advance(done, avail, m, max_new)
        history.append(list(done))
        assert list(host(answered)) == done, (r, list(host(answered)), done)
        assert list(host(rank)) == [model(o, done[o])[1] for o in range(nobj)], r
        check_snapshot(stream, model, done, r)
    return stream, pieces, model, history


def test_small_shape_block_larger_than_m(ctx1):
    k, m = 16, 20
    assert ls.large_block(k, m) == 32 > m
    rng = np.random.default_rng(1620)
    co = np.stack([ls.planted(rng, k, m), sparse_vectors(rng, k, m, 2), rng.integers(0, 256, (m, k), dtype=np.uint8)])
    _, _, model, hist = run_schedule(ctx1, k, co, [
        ([3, 20, 0], None),    # one object complete in one push, one untouched
        ([3, 25, 7], None),    # nothing new; avail above m; a first push
        ([11, 2, 7], 5),       # max_new caps the first (3 -> 8); avail below done; nothing new
        ([20, 20, 20], None),
        ([20, 20, 20], None),  # nothing left for anyone
    ])
    assert hist == [[0, 0, 0], [3, 20, 0], [3, 20, 7], [8, 20, 7], [20, 20, 20], [20, 20, 20]]
    assert model(2, 20)[1] == k and RECEIVED_ALL in model(2, 20)[0]


def test_block_boundaries_and_idle_objects(ctx1):
    """(24, 67), B = 32, m no multiple of 4; the three objects of block_cases (a zero piece, a duplicate and a multiple on
    the block boundaries; objects b and c reach rank k inside a block)."""
    k, m, B = 24, 67, 32
    assert ls.large_block(k, m) == B
    co = block_cases(np.random.default_rng(m), k, m, B)
    _, _, model, hist = run_schedule(ctx1, k, co, [
        ([5, 32, 0], None),     # b: exactly B new pieces, rank k inside the block, the rest of it ReceivedAllPieces
        ([9, 65, 15], B),       # a: new rows on top of stored ones; b: B + 1 new with max_new = B, one is left over
        ([9, 65, 40], None),    # a: idle right after gaining rows while the others advance; b: the one left over,
                                # answered at rank k by a later push
        ([42, 200, 40], 7),     # a: max_new no multiple of 4; b: avail above m; c: idle right after gaining rows
        ([3, 67, 67], None),    # a: avail below done
        ([67, 67, 67], B),      # a: exactly B new pieces from the middle of a block of the one-shot form
        ([67, 67, 67], None),
    ])
    assert hist == [[0, 0, 0], [5, 32, 0], [9, 64, 15], [9, 65, 40], [16, 67, 40], [16, 67, 67], [48, 67, 67],
                    [67, 67, 67]]
    # the inputs do what the schedule needs
    assert model(0, 5)[1] >= 3 and model(0, 9)[1] > model(0, 5)[1]  # a gained rows on top of stored ones, then idled
    sb = model(1, 32)[0]
    assert model(1, 32)[1] == k and RECEIVED_ALL in sb and sb.index(RECEIVED_ALL) < B - 1
    assert model(1, 67)[0][32:] == [RECEIVED_ALL] * 35
    assert model(2, 40)[1] > model(2, 15)[1] and model(2, 67)[1] == k
    assert model(0, 67)[0][1] == NOT_USEFUL and model(0, 67)[0][B] == NOT_USEFUL and model(2, 67)[0][B] == NOT_USEFUL


@pytest.mark.parametrize("k,m", [(24, 67), (16, 20)])
def test_one_push_of_everything_is_the_one_shot_elimination(ctx1, k, m):
    import torch

    from rlnc_amd import batch

    B = ls.large_block(k, m)
    co = block_cases(np.random.default_rng(m + 1), k, m, B) if m > B else \
        np.stack([sparse_vectors(np.random.default_rng(s), k, m, 3) for s in range(3)])
    pieces = pieces_of(co, seed=5)
    nobj = co.shape[0]
    stream = batch.DecodeStream(k, m, nobj, ctx1)
    stream.push(pieces, torch.full((nobj,), m, dtype=torch.int32, device="cuda:0"), m)
    got = (torch.full((nobj, k, m), 0xAA, dtype=torch.uint8, device="cuda:0"), i32((nobj, m)), i32(nobj))
    stream.snapshot(*got)
    want = (torch.full((nobj, k, m), 0x55, dtype=torch.uint8, device="cuda:0"), i32((nobj, m), -9), i32(nobj, -9))
    ctx1.set_decode_path(LARGE)
    try:
        batch.decode_batch_eliminate(pieces, k, *want, ctx1)
    finally:
        ctx1.set_decode_path(0)
    for g, w in zip(got, want):
        assert np.array_equal(host(g), host(w))
    assert (host(got[1]) != PENDING).all()


def test_beyond_lds_dense(ctx1):
    k, m = 300, 310
    rng = np.random.default_rng(300310)
    co = np.stack([ls.planted3(rng, k, m) for _ in range(3)])
    _, _, model, hist = run_schedule(ctx1, k, co, [
        ([150, 310, 40], None),   # b: everything at once, ten blocks
        ([190, 310, 200], 64),    # a: new rows on top of stored ones (two blocks, the second partial); c: capped
        ([190, 310, 310], None),  # a: idle right after gaining rows
        ([310, 310, 310], None),
    ])
    assert hist[2] == [190, 310, 104] and hist[-1] == [310, 310, 310]
    for o in range(3):
        st, rank, _, _ = model(o, m)
        assert rank == k and st.count(NOT_USEFUL) == 3 and st[-1] == RECEIVED_ALL


def test_block_of_28(ctx1):
    """(40, 4796): rows so wide that a block is 28 pieces, a multiple of 4 that is not 32.  The trickle input keeps the
    model cheap; only the first slots of the 4796 are filled."""
    k, m, B = 40, M28, 28
    assert ls.large_block(k, m) == B
    rng = np.random.default_rng(4796)
    co = np.stack([ls.trickle(rng, k, m, B, 36), ls.trickle(rng, k, m, B, 40, last_at=m // 2 + 3),
                   ls.trickle(rng, k, m, B, 40)])
    _, _, model, hist = run_schedule(ctx1, k, co, [
        ([B, B + 1, 10], B),      # exactly B; B + 1 with max_new = B
        ([B, B + 1, 75], None),   # idle; the one left over; three blocks, the last partial
        ([100, 20, 75], 30),      # max_new no multiple of 4 and more than a block; avail below done; idle
        ([100, 60, 80], None),
    ])
    assert hist == [[0, 0, 0], [28, 28, 10], [28, 29, 75], [58, 29, 75], [100, 60, 80]]
    assert NOT_USEFUL in model(0, 100)[0] and model(2, 75)[1] > model(2, 10)[1]


def test_m_far_below_the_block(ctx1):
    k, m = 2000, 8
    assert ls.large_block(k, m) == 32
    rng = np.random.default_rng(2008)
    co = np.stack([ls.trickle(rng, k, m, 32, m) for _ in range(3)])
    _, _, model, hist = run_schedule(ctx1, k, co, [([3, 8, 0], None), ([3, 9, 5], 3), ([8, 8, 8], None)])
    assert hist == [[0, 0, 0], [3, 8, 0], [3, 8, 3], [8, 8, 8]]
    assert NOT_USEFUL in model(1, 8)[0]


def test_end_to_end(ctx1):
    """Encode with the library, deliver the pieces over rounds, apply: NotAllPiecesReceivedYet for the objects still
    short of rank k, then decoded == source."""
    import torch

    from rlnc_amd import batch

    k, L, m, nobj = 24, 256, 40, 3
    rng = np.random.default_rng(77)
    datas = [rng.integers(0, 256, k * L - 1 - 5 * o, dtype=np.uint8) for o in range(nobj)]
    src = np.stack([npo.pad(d, k) for d in datas])
    co = rng.integers(0, 256, (nobj, m, k), dtype=np.uint8)
    co[1, 3] = co[1, 1]  # a useless arrival: object 1 needs k + 1 slots
    sent = torch.zeros((nobj, m, k + L), dtype=torch.uint8, device="cuda:0")
    batch.encode_batch(dev(src), dev(co), sent, ctx1)
    pieces = torch.zeros_like(sent)  # the receiver's slots, filled as pieces arrive
    stream = batch.DecodeStream(k, m, nobj, ctx1)
    decoded = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0")
    ost, dl = i32(nobj), torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0")
    rank, avail = i32(nobj), torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
    filled = [0] * nobj
    for arrivals in ([10, 24, 3], [20, 24, 14], [24, 25, 23], [24, 25, 24]):
        for o, n in enumerate(arrivals):
            pieces[o, filled[o]:n] = sent[o, filled[o]:n]
            filled[o] = n
        avail.copy_(torch.tensor(arrivals, dtype=torch.int32))
        stream.push(pieces, avail, rank=rank)
        want_rank = [true_rank_model(k, co[o, :n])[1] for o, n in enumerate(arrivals)]
        assert list(host(rank)) == want_rank, arrivals
        stream.apply(pieces, decoded, ost, dl)
        for o in range(nobj):
            if want_rank[o] < k:
                assert host(ost)[o] == NOT_ALL_YET and host(dl)[o] == 0, (arrivals, o)
            else:
                assert host(ost)[o] == OK and int(host(dl)[o]) == datas[o].size, (arrivals, o)
                assert np.array_equal(host(decoded)[o], src[o]), (arrivals, o)
    assert list(host(rank)) == [k] * nobj and true_rank_model(k, co[1, :24])[1] == k - 1


# ---- refusals: every one on the host, before a launch ------------------------------------------------------------------


def test_refusals(ctx1):
    import torch

    import rlnc_amd
    from rlnc_amd import batch
    from rlnc_amd.errors import RLNCError

    k, m, nobj, L = 12, 21, 3, 4  # a shape no other test initialises: the library knows a state by its address
    nbytes = batch.state_bytes(k, m, nobj)
    pieces = pieces_of(np.random.default_rng(3).integers(0, 256, (nobj, m, k), dtype=np.uint8))
    avail = torch.full((nobj,), m, dtype=torch.int32, device="cuda:0")
    buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    state, pp, ap = C.c_void_p(buf.data_ptr()), C.c_void_p(pieces.data_ptr()), C.c_void_p(avail.data_ptr())

    def push(st=state, n=nbytes, k_=k, m_=m, nobj_=nobj, ctx=ctx1, L_=L, max_new=m):
        return raw(ctx, "rlnc_decode_stream_push", st, n, pp, 0, k_, L_, m_, nobj_, ap, max_new, None, None)

    # a state that was never initialised
    assert push() == INVALID
    assert raw(ctx1, "rlnc_decode_stream_snapshot", state, nbytes, k, m, nobj, None, None, None) == INVALID
    # rank mode 0: init, push and snapshot
    ctx0 = rlnc_amd.Context(0)
    assert raw(ctx0, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == INVALID
    with pytest.raises(RLNCError) as ei:
        batch.DecodeStream(k, m, nobj, ctx0)
    assert ei.value == RLNCError.InvalidArgument
    # short or misaligned by 4 bytes
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes - 16, k, m, nobj) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_init", C.c_void_p(buf.data_ptr() + 4), nbytes, k, m, nobj) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_init", None, nbytes, k, m, nobj) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, 4097, m, nobj) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
    assert push(ctx=ctx0) == INVALID and raw(ctx0, "rlnc_decode_stream_snapshot", state, nbytes, k, m, nobj, None,
                                             None, None) == INVALID
    assert push(n=nbytes - 16) == INVALID and push(st=C.c_void_p(buf.data_ptr() + 4)) == INVALID
    # other values than init's (each a shape whose state fits the buffer)
    assert push(k_=k - 1) == INVALID and push(m_=m - 1) == INVALID and push(nobj_=nobj - 1) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_snapshot", state, nbytes, k, m - 1, nobj, None, None, None) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, None, 0, k, L, m, nobj, ap, m, None, None) == INVALID
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, pp, 0, k, L, m, nobj, None, m, None, None) == INVALID
    # the crate's checks, in order, and the calls that have nothing to do
    assert push(k_=0, L_=0) == 3 and push(L_=0) == 5
    assert push(max_new=0) == 0 and push(nobj_=0) == 0
    torch.cuda.synchronize()
    # nothing of the above touched the stream: everything is still pending, and it works
    ps = i32((nobj, m))
    assert raw(ctx1, "rlnc_decode_stream_snapshot", state, nbytes, k, m, nobj, None, C.c_void_p(ps.data_ptr()),
               None) == 0
    assert (host(ps) == PENDING).all()
    assert push() == 0
    assert raw(ctx1, "rlnc_decode_stream_snapshot", state, nbytes, k, m, nobj, None, C.c_void_p(ps.data_ptr()),
               None) == 0
    assert (host(ps) != PENDING).all()
    assert not host(buf)[nbytes:].any()


# ---- footprint ---------------------------------------------------------------------------------------------------------

def test_footprint(ctx1):
    """Push writes the state (within state_bytes), rank and answered, nothing else; snapshot writes all of T, the
    statuses and the rank and leaves the state as it was."""
    import torch

    from rlnc_amd import batch

    k, m, nobj, L, B = 24, 67, 3, 4, 32
    co = block_cases(np.random.default_rng(9), k, m, B)
    model = Prefixes(k, co)
    nbytes = batch.state_bytes(k, m, nobj)
    sa = Arena(nbytes, seed=120)
    sa.device()
    state = C.c_void_p(sa.region().data_ptr())
    host_pieces = host(pieces_of(co, L, seed=6))
    pieces = dev(host_pieces)
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
    done = [0] * nobj
    for r, (avail, max_new) in enumerate([([40, 67, 3], 33), ([40, 67, 3], 33), ([67, 67, 50], 67)]):
        host_avail = np.array(avail, np.int32)
        av = torch.from_numpy(host_avail.copy()).to("cuda:0")
        done = advance(done, avail, m, max_new)
        oa = Arena(2 * nobj * 4, seed=130 + r)
        oa.operand("rank", 0, 1, 0, nobj, 4, 4)
        oa.operand("answered", nobj * 4, 1, 0, nobj, 4, 4)
        oa.expect("rank", np.array([model(o, done[o])[1] for o in range(nobj)], np.int32))
        oa.expect("answered", np.array(done, np.int32))
        oa.device()
        assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, C.c_void_p(pieces.data_ptr()), 0, k, L, m, nobj,
                   C.c_void_p(av.data_ptr()), max_new, C.c_void_p(oa.ptr("rank")), C.c_void_p(oa.ptr("answered"))) == 0
        oa.check_device()
        sa.check_guards(sa.after())
        assert_inputs_unchanged({"pieces": (host_pieces, pieces), "avail": (host_avail, av)})
        # the snapshot: every byte of its outputs, none of the state
        before = sa.after()
        ta = Arena(nobj * k * m, seed=140 + r, base_off=r)  # T at any byte alignment
        ta.operand("T", 0, nobj, k * m, k, m, m)
        Tm = np.zeros((nobj, k, m), np.uint8)
        st = np.full((nobj, m), PENDING, np.int32)
        for o in range(nobj):
            s, _, To, _ = model(o, done[o])
            Tm[o][:, :done[o]] = To
            st[o, :done[o]] = s
        ta.expect("T", Tm)
        ta.device()
        pa = Arena(nobj * m * 4 + nobj * 4, seed=150 + r)
        pa.operand("status", 0, nobj, m * 4, m, 4, 4)
        pa.operand("rank", nobj * m * 4, 1, 0, nobj, 4, 4)
        pa.expect("status", st)
        pa.expect("rank", np.array([model(o, done[o])[1] for o in range(nobj)], np.int32))
        pa.device()
        assert raw(ctx1, "rlnc_decode_stream_snapshot", state, nbytes, k, m, nobj, C.c_void_p(ta.ptr("T")),
                   C.c_void_p(pa.ptr("status")), C.c_void_p(pa.ptr("rank"))) == 0
        ta.check_device()
        pa.check_device()
        assert np.array_equal(sa.after(), before), "the snapshot wrote into the state"
    assert done == [67, 67, 50]


# ---- graph capture -----------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch
from tests.limit_shapes import block_cases

k, m, B, L = 24, 67, 32, 4
co = block_cases(np.random.default_rng(31), k, m, B)
nobj = co.shape[0]
p = np.random.default_rng(1).integers(0, 256, (nobj, m, k + L), dtype=np.uint8)
p[:, :, :k] = co
pieces = torch.from_numpy(p).cuda()
ctx = rlnc_amd.Context(0)
ctx.set_rank_mode(1)
rounds = [[5, 32, 0], [9, 65, 15], [9, 65, 40], [42, 200, 40], [67, 67, 67], [67, 67, 67], [67, 67, 67]]


def snapshot(s):
    out = (torch.full((nobj, k, m), 0xAA, dtype=torch.uint8, device="cuda"),
           torch.full((nobj, m), -7, dtype=torch.int32, device="cuda"),
           torch.full((nobj,), -7, dtype=torch.int32, device="cuda"))
    s.snapshot(*out)
    torch.cuda.synchronize()
    return out


eager = batch.DecodeStream(k, m, nobj, ctx)
avail = torch.zeros(nobj, dtype=torch.int32, device="cuda")
for r in rounds:  # the eager stream, and the eager push before any capture
    avail.copy_(torch.tensor(r, dtype=torch.int32))
    eager.push(pieces, avail, B)
torch.cuda.synchronize()
want = snapshot(eager)
assert (want[1].cpu().numpy() != -1).all()

cap = batch.DecodeStream(k, m, nobj, ctx)
rank = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
answered = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
avail.zero_()
torch.cuda.synchronize()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap.push(pieces, avail, B, rank, answered)
done = [0] * nobj
for r in rounds:
    avail.copy_(torch.tensor(r, dtype=torch.int32))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    done = [min(max(a, d), m, d + B) for d, a in zip(done, r)]
    assert answered.cpu().tolist() == done, (answered.cpu().tolist(), done)
assert done == [m] * nobj
got = snapshot(cap)
for a, b in zip(got, want):
    assert torch.equal(a, b), "the replayed stream differs from the eager one"
assert rank.cpu().tolist() == got[2].cpu().tolist()
print("stream graph ok")
"""


def test_push_under_graph_capture():
    """One eager push first, then one push with max_new = B captured (a linear graph) and replayed over the rounds
    while avail changes between replays: the final snapshot equals the eager stream's."""
    code = CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream graph ok" in r.stdout
