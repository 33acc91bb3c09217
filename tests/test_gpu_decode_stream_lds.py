"""GPU: the LDS form of a decode stream's push (include/rlnc_hip.h, rlnc_set_stream_form; rlnc_amd/csrc/rank_stream.hip)
against the numpy model of tests/true_rank.py run on each object's own prefix, with the helpers of
tests/stream_util.py.  All comparisons are exact.

Under form 2 a snapshot after every push must be the model of the slots pushed so far (T, statuses with PENDING, rank),
and so must the push's own rank / answered arrays.  The two forms alternated push by push must leave the live state --
state words 0 and 2, piv[0..rank), St[0..done), R[0..rank)[D] -- byte for byte what the workspace form alone leaves:
that pins the coefficient half of the rows, which T does not show.  A push writes only the ranges rank_stream.hip names.

The shapes: (1, 1); (5, 7) odd kd, m no multiple of 4; (24, 40); (32, 32) m = k; (4, 1100) rows of 276 dwords, more
than a workgroup's threads; the largest m that fits LDS at k = 200; 1,027 objects of (8, 12) for the one-wave-per-object
arrangement with a last workgroup of three valid waves."""
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
from tests.stream_util import (Prefixes, advance, check_snapshot, i32, live_state, pieces_of, raw, state_words,
                               true_rank_context)
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL, sparse_vectors, true_rank_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 100
AUTO, WORKSPACE, LDS = 0, 1, 2
K200 = [fit for fit, _ in ls.RANK_EDGES if fit[0] == 200][0]  # (200, the largest m that fits)
BEYOND16 = [beyond for fit, beyond in ls.RANK_EDGES if fit[0] == 16][0]  # the first shape beyond LDS at k = 16


@pytest.fixture(scope="module")
def ctx1():
    return true_rank_context()


def inputs(rng, k, m):
    """Four objects [4][m][k]: a dense with an all-zero piece and a repeated one; b sparse (sparse_vectors), and where
    m is far above k all zero but for k slots spread over the m, so that rows are inserted at high slot indices; c
    dense with planted duplicates, multiples and sums; d dense."""
    a = rng.integers(0, 256, (m, k), dtype=np.uint8)
    if m > 3:
        a[1] = 0
        a[3] = a[2]
    b = sparse_vectors(rng, k, m, 2)
    if m > 4 * k:  # k independent vectors (triangular), the last one in the last slot
        b[:] = 0
        for i, t in enumerate(list(np.sort(rng.choice(m - 1, size=k - 1, replace=False))) + [m - 1]):
            b[t, i] = rng.integers(1, 256)
            b[t, max(i - 1, 0)] ^= rng.integers(0, 256) if i else 0
    c = ls.planted(rng, k, m) if m > 3 else rng.integers(0, 256, (m, k), dtype=np.uint8)
    d = rng.integers(1, 256, (m, k), dtype=np.uint8)
    return np.stack([a, b, c, d])


def schedule(m):
    """[(avail of a, b, c, d; max_new)] -- what each round is there for:"""
    return [
        ([m + 7, 1, 0, 0], None),       # a: everything in one push, avail above m, rank k inside the push; c, d idle
        ([0, 2, 3, 0], 1),              # a: avail below done; b: one piece per push; c: max_new = 1 caps; d idle
        ([m, m, m, 0], 3),              # max_new = 3; a has nothing left
        ([m, m, m, 0], 5),              # max_new = 5
        ([m, m, m, 2], None),           # b, c: the rest at once; d: a first push
        ([m, m, m, max(m - 2, 2)], None),  # a, b, c idle for good; d reaches rank k inside the push where m >= k + 4
        ([m, m, m, m], 1),              # d: a push after rank k, one slot
        ([m, m, m, m], None),           # d: the last slot
        ([m, m, m, m], None),           # nothing left for anyone
    ]


def run(ctx, k, co, rounds, form_of):
    """The rounds on one stream, push r under form form_of(r).  After every push: rank / answered of the push and a
    snapshot against the model of each object's prefix.  avail is overwritten right after the push is enqueued."""
    import torch

    from rlnc_amd import batch

    nobj, m, _ = co.shape
    pieces = pieces_of(co, seed=k + m)
    model = Prefixes(k, co)
    stream = batch.DecodeStream(k, m, nobj, ctx)
    done = [0] * nobj
    try:
        for r, (avail, max_new) in enumerate(rounds):
            ctx.set_stream_form(form_of(r))
            av = torch.tensor(avail, dtype=torch.int32, device="cuda:0")
            rank, answered = i32(nobj), i32(nobj)
            stream.push(pieces, av, max_new, rank, answered)
            av.fill_(m + 12345)  # every object read its avail in the push's launch: nothing reads it any more
            done = advance(done, avail, m, max_new)
            assert list(host(answered)) == done, (r, list(host(answered)), done)
            assert list(host(rank)) == [model(o, done[o])[1] for o in range(nobj)], r
            check_snapshot(stream, model, done, r)
    finally:
        ctx.set_stream_form(AUTO)
    return stream, model, done


@pytest.mark.parametrize("k,m", [(1, 1), (5, 7), (24, 40), (32, 32), (4, 1100)])
def test_lds_form_against_the_model(ctx1, k, m):
    co = inputs(np.random.default_rng(1000 * k + m), k, m)
    _, model, done = run(ctx1, k, co, schedule(m), lambda r: LDS)
    assert done == [m] * 4
    if m >= k + 4:  # the inputs do what the schedule needs
        sa = model(0, m)[0]
        assert model(0, m)[1] == k and sa[1] == NOT_USEFUL and sa[3] == NOT_USEFUL and RECEIVED_ALL in sa
        assert model(3, m - 2)[1] == k and model(3, m)[0][-2:] == [RECEIVED_ALL] * 2
        assert NOT_USEFUL in model(2, m)[0]
    if m > 4 * k:  # rows inserted at slots whose unit byte lies beyond dword 256 of the row
        sb = model(1, m)[0]
        assert sb[-1] == OK and model(1, m)[1] == k and sb.count(NOT_USEFUL) == m - k


def test_lds_form_at_the_largest_shape_that_fits(ctx1):
    k, m = K200
    assert ls.rank_lds_bytes(k, m) <= ls.MAX_LDS < ls.rank_lds_bytes(k, m + 1)
    rng = np.random.default_rng(200)
    co = np.stack([ls.planted3(rng, k, m), sparse_vectors(rng, k, m, 3)])
    _, model, done = run(ctx1, k, co, [
        ([150, 1], None),
        ([151, 2], 1),          # one piece on top of 150 stored rows
        ([m + 3, 100], 5),
        ([m, m], None),         # a: rank k inside the push, the last slots ReceivedAllPieces
        ([m, m], None),
    ], lambda r: LDS)
    assert done == [m, m]
    assert model(0, m)[1] == k and model(0, m)[0][-1] == RECEIVED_ALL


def wave_inputs(nobj=1027, k=8, m=12):
    rng = np.random.default_rng(1027)
    co = rng.integers(0, 256, (nobj, m, k), dtype=np.uint8)
    co[1::5] = np.stack([sparse_vectors(rng, k, m, 2) for _ in range(len(co[1::5]))])
    co[2::7, 1] = 0
    co[3::7, 4] = co[3::7, 2]
    rounds = []
    for max_new in (None, 1, 3, 5, None, None):
        avail = rng.integers(-2, m + 4, nobj)
        avail[::9] = 0  # idle for as long as this holds
        rounds.append(([int(a) for a in avail], max_new))
    rounds[-2] = ([m] * nobj, None)
    rounds[-1] = ([m] * nobj, None)
    return k, co, rounds


def test_lds_form_one_wave_per_object(ctx1):
    """1,027 objects of (8, 12): k <= 16, D = 5 <= 16 and >= 1,024 objects, so four objects share a workgroup and the
    last workgroup has one wave without an object."""
    k, co, rounds = wave_inputs()
    _, model, done = run(ctx1, k, co, rounds, lambda r: LDS)
    assert done == [12] * 1027
    assert any(model(o, 12)[1] < k for o in range(1027)) and any(RECEIVED_ALL in model(o, 12)[0] for o in range(1027))


@pytest.mark.parametrize("form", [AUTO, WORKSPACE])
def test_the_other_forms_on_the_same_schedule(ctx1, form):
    k, m = 24, 40
    co = inputs(np.random.default_rng(1000 * k + m), k, m)
    _, _, done = run(ctx1, k, co, schedule(m), lambda r: form)
    assert done == [m] * 4


def mixed_against_workspace(ctx, k, co, rounds, with_model):
    import torch

    from rlnc_amd import batch

    nobj, m, _ = co.shape
    pieces = pieces_of(co, seed=3)
    model = Prefixes(k, co)
    ref, mix = batch.DecodeStream(k, m, nobj, ctx), batch.DecodeStream(k, m, nobj, ctx)
    done = [0] * nobj
    try:
        for r, (avail, max_new) in enumerate(rounds):
            av = torch.tensor(avail, dtype=torch.int32, device="cuda:0")
            ctx.set_stream_form(WORKSPACE)
            ref.push(pieces, av, max_new)
            ctx.set_stream_form(LDS if r % 2 == 0 else WORKSPACE)
            mix.push(pieces, av, max_new)
            done = advance(done, avail, m, max_new)
            a, b = live_state(host(ref.state), k, m, nobj), live_state(host(mix.state), k, m, nobj)
            for o in range(nobj):
                assert a[o][:2] == b[o][:2] and a[o][1] == done[o], (r, o, a[o][:2], b[o][:2], done[o])
                for what, x, y in zip(("piv", "St", "R"), a[o][2:], b[o][2:]):
                    assert x == y, (r, o, what)
            snaps = []
            for s in (ref, mix):
                out = (torch.full((nobj, k, m), 0xAA, dtype=torch.uint8, device="cuda:0"), i32((nobj, m)), i32(nobj))
                s.snapshot(*out)
                snaps.append([host(t) for t in out])
            for x, y in zip(*snaps):
                assert np.array_equal(x, y), r
            if with_model:
                check_snapshot(mix, model, done, r)
    finally:
        ctx.set_stream_form(AUTO)
    return done


def test_forms_mixed_push_by_push(ctx1):
    """One state buffer under forms 2, 1, 2, ... against one under form 1 throughout: the same live state after every
    push, coefficient halves of the rows included.  The form-1 arm alone runs on a library without the LDS form."""
    k, m = 24, 40
    co = inputs(np.random.default_rng(2440), k, m)
    assert mixed_against_workspace(ctx1, k, co, schedule(m), True) == [m] * 4
    # the same with the LDS pushes at the odd rounds: drop the first round
    assert mixed_against_workspace(ctx1, k, co, schedule(m)[1:], False) == [m] * 4


def test_forms_mixed_one_wave_per_object(ctx1):
    k, co, rounds = wave_inputs()
    assert mixed_against_workspace(ctx1, k, co, rounds, False) == [12] * 1027


# ---- set_stream_form and the refusals ----------------------------------------------------------------------------------

def test_set_stream_form_and_refusals(ctx1):
    import torch

    import rlnc_amd
    from rlnc_amd import batch
    from rlnc_amd.errors import RLNCError

    k, m = BEYOND16
    nobj, L = 2, 4
    assert not batch.stream_lds_fits(k, m) and batch.stream_lds_fits(k, m - 1)
    nbytes = batch.state_bytes(k, m, nobj)
    pieces = pieces_of(sparse_vectors(np.random.default_rng(4), k, nobj * m, 2).reshape(nobj, m, k), L)
    avail = torch.full((nobj,), 9, dtype=torch.int32, device="cuda:0")
    buf = dev(np.random.default_rng(5).integers(0, 256, nbytes, dtype=np.uint8))
    state, pp, ap = C.c_void_p(buf.data_ptr()), C.c_void_p(pieces.data_ptr()), C.c_void_p(avail.data_ptr())

    def push(ctx=ctx1):
        return raw(ctx, "rlnc_decode_stream_push", state, nbytes, pp, 0, k, L, m, nobj, ap, m, None, None)

    try:
        assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
        before = host(buf).copy()
        for form in (AUTO, WORKSPACE, LDS):
            assert raw(ctx1, "rlnc_set_stream_form", form) == 0
        # form 2 on the first shape beyond LDS: refused, the limit named, the state untouched; other values leave form 2
        assert raw(ctx1, "rlnc_set_stream_form", 3) == INVALID and raw(ctx1, "rlnc_set_stream_form", -1) == INVALID
        assert push() == INVALID
        assert str(ls.MAX_LDS).encode() in ctx1.lib.rlnc_last_error()
        assert np.array_equal(host(buf), before)
        with pytest.raises(RLNCError) as ei:
            ctx1.set_stream_form(7)
        assert ei.value == RLNCError.InvalidArgument
        assert push() == INVALID
        # ... and leave form 1 when that was set: the workspace form takes the shape
        ctx1.set_stream_form(WORKSPACE)
        assert raw(ctx1, "rlnc_set_stream_form", 3) == INVALID
        assert push() == 0
        torch.cuda.synchronize()
        assert [int(w[2]) for w in state_words(host(buf), k, m, nobj)] == [9, 9]
        # a context in rank mode 0 is refused as before, whatever its form
        ctx0 = rlnc_amd.Context(0)
        for form in (AUTO, WORKSPACE, LDS):
            ctx0.set_stream_form(form)
            assert push(ctx0) == INVALID
            assert b"rank mode" in ctx0.lib.rlnc_last_error()
    finally:
        ctx1.set_stream_form(AUTO)


# ---- footprint ---------------------------------------------------------------------------------------------------------

def test_footprint(ctx1):
    """A form-2 push writes St[done..target), piv[0..rank') and R[0..rank')[D] when a row was inserted, and the four
    state words; Q, X, the rows and statuses past the live range, every word of an idle object and the guards around the
    state keep their (random) prefill.  rank and answered are written for every object, idle ones included."""
    import torch

    from rlnc_amd import batch

    k, m, nobj, L = 24, 40, 4, 4
    lay = ls.large_layout(k, m)
    co = inputs(np.random.default_rng(77), k, m)
    co[3, 5] = co[3, 4]  # d's round-3 push inserts nothing
    model = Prefixes(k, co)
    nbytes = batch.state_bytes(k, m, nobj)
    sa = Arena(nbytes, seed=220)
    sa.device()
    state = C.c_void_p(sa.region().data_ptr())
    host_pieces = host(pieces_of(co, L, seed=6))
    pieces = dev(host_pieces)
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
    done = [0] * nobj
    rounds = [([m, 3, 0, 5], None),    # a: rank k inside the push; c idle from the start
              ([m, 3, 0, 5], None),    # everyone idle: not a byte of the state changes
              ([m, 9, 2, 6], 4),       # d: one useless piece -- statuses and state words only
              ([m, m, m, m], None),
              ([m, m, m, m], None)]
    ctx1.set_stream_form(LDS)
    try:
        for r, (avail, max_new) in enumerate(rounds):
            before = state_words(sa.after()[sa.start: sa.end], k, m, nobj).copy()
            host_avail = np.array(avail, np.int32)
            av = torch.from_numpy(host_avail.copy()).to("cuda:0")
            new = advance(done, avail, m, max_new)
            ranks = [(model(o, done[o])[1], model(o, new[o])[1]) for o in range(nobj)]
            oa = Arena(2 * nobj * 4, seed=230 + r)
            oa.operand("rank", 0, 1, 0, nobj, 4, 4)
            oa.operand("answered", nobj * 4, 1, 0, nobj, 4, 4)
            oa.expect("rank", np.array([r1 for _, r1 in ranks], np.int32))
            oa.expect("answered", np.array(new, np.int32))
            oa.device()
            assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, C.c_void_p(pieces.data_ptr()), 0, k, L, m, nobj,
                       C.c_void_p(av.data_ptr()), m if max_new is None else max_new, C.c_void_p(oa.ptr("rank")),
                       C.c_void_p(oa.ptr("answered"))) == 0
            oa.check_device()
            image = sa.after()
            sa.check_guards(image)
            assert_inputs_unchanged({"pieces": (host_pieces, pieces), "avail": (host_avail, av)})
            after = state_words(image[sa.start: sa.end], k, m, nobj)
            for o in range(nobj):
                (r0, r1), d0, d1 = ranks[o], done[o], new[o]
                may = np.zeros(lay["total"], bool)
                if d1 > d0:
                    may[:4] = True
                    may[lay["st"] + d0: lay["st"] + d1] = True
                    if r1 > r0:
                        may[lay["piv"]: lay["piv"] + r1] = True
                        may[lay["r"]: lay["r"] + r1 * lay["D"]] = True
                    assert list(after[o][:4]) == [r1, r1, d1, d1], (r, o)
                    assert list(after[o][lay["st"] + d0: lay["st"] + d1].view(np.int32)) == model(o, d1)[0][d0:], (r, o)
                stray = np.flatnonzero((after[o] != before[o]) & ~may)
                assert stray.size == 0, (r, o, "dword", int(stray[0]), "of", lay)
            if r == 1:
                assert new == done and np.array_equal(after, before)
            if r == 2:
                assert ranks[3][0] == ranks[3][1] and new[3] == done[3] + 1
            done = new
    finally:
        ctx1.set_stream_form(AUTO)
    assert done == [m] * nobj


# ---- end to end --------------------------------------------------------------------------------------------------------

def test_end_to_end(ctx1):
    """Encode with the library, deliver the pieces over rounds under form 2, apply: decoded == source, with lengths."""
    import torch

    from rlnc_amd import batch

    k, L, m, nobj = 24, 4, 40, 3
    rng = np.random.default_rng(78)
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
    ctx1.set_stream_form(LDS)
    try:
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
                    assert host(ost)[o] == 10 and host(dl)[o] == 0, (arrivals, o)
                else:
                    assert host(ost)[o] == OK and int(host(dl)[o]) == datas[o].size, (arrivals, o)
                    assert np.array_equal(host(decoded)[o], src[o]), (arrivals, o)
    finally:
        ctx1.set_stream_form(AUTO)
    assert list(host(rank)) == [k] * nobj and true_rank_model(k, co[1, :24])[1] == k - 1


# ---- graph capture -----------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch
from tests.limit_shapes import block_cases
from tests.true_rank import true_rank_model

k, m, B, L = 24, 40, 8, 4
co = block_cases(np.random.default_rng(32), k, 3 * B, B)
co = np.concatenate([co, np.random.default_rng(33).integers(0, 256, (3, m - 3 * B, k), dtype=np.uint8)], axis=1)
nobj = co.shape[0]
p = np.random.default_rng(1).integers(0, 256, (nobj, m, k + L), dtype=np.uint8)
p[:, :, :k] = co
pieces = torch.from_numpy(p).cuda()
ctx = rlnc_amd.Context(0)
ctx.set_rank_mode(1)
ctx.set_stream_form(2)
rounds = [[5, 8, 0], [9, 30, 15], [9, 30, 15], [3, 200, 16], [40, 40, 40], [40, 40, 40], [40, 40, 40], [40, 40, 40]]

avail = torch.full((nobj,), 2, dtype=torch.int32, device="cuda")
batch.DecodeStream(k, m, nobj, ctx).push(pieces, avail)  # the form's first launch comes before any capture
cap = batch.DecodeStream(k, m, nobj, ctx)
rank = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
answered = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
avail.zero_()
torch.cuda.synchronize()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap.push(pieces, avail, 13, rank, answered)
T = torch.empty((nobj, k, m), dtype=torch.uint8, device="cuda")
ps = torch.empty((nobj, m), dtype=torch.int32, device="cuda")
done = [0] * nobj
for r in rounds:
    avail.copy_(torch.tensor(r, dtype=torch.int32))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    done = [min(max(a, d), m, d + 13) for d, a in zip(done, r)]
    assert answered.cpu().tolist() == done, (answered.cpu().tolist(), done)
    T.fill_(0xAA)
    ps.fill_(-7)
    cap.snapshot(T, ps)
    torch.cuda.synchronize()
    for o in range(nobj):
        st, rk, Tm, _ = true_rank_model(k, co[o, :done[o]]) if done[o] else ([], 0, np.zeros((k, 0), np.uint8), None)
        assert ps[o].cpu().tolist() == st + [-1] * (m - done[o]), (r, o)
        assert int(rank[o]) == rk, (r, o)
        assert np.array_equal(T[o].cpu().numpy()[:, :done[o]], Tm) and not T[o].cpu().numpy()[:, done[o]:].any(), (r, o)
assert done == [m] * nobj
print("stream lds graph ok")
"""


def test_push_under_graph_capture():
    """A form-2 push with max_new = 13 captured once (one kernel node) and replayed while avail changes between
    replays: the model of each object's prefix after every replay."""
    code = CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream lds graph ok" in r.stdout
