"""GPU: a decode stream's accept (include/rlnc_hip.h, rlnc_decode_stream_accept; rlnc_amd/csrc/stream_accept.hip;
rlnc_amd.batch.DecodeStream.accept) against the numpy model of tests/accept_util.py, whose patterns
tests/test_decode_stream_accept_host.py holds to their names.  All comparisons are exact.

An accept must put arrival j of object o, in arrival order, into slot a + j of the object's pieces while a + j < m, a =
avail[o] clamped to [0, m]; answer NoRoom, NoObject, Finished or Absent for the others and copy nothing of them; rewrite
avail and refused; and touch no other byte."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests import accept_util as au
from tests.accept_util import ABSENT, FINISHED, NO_OBJECT, NO_ROOM, accept_model, pattern, place
from tests.deliver_util import independent
from tests.far_address import FAR_ODD, FarArena, FarLayout
from tests.footprint import Arena, assert_inputs_unchanged
from tests.gpu_util import dev, host, np_matmul
from tests.stream_util import live_state, raw, true_rank_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 100
WORKSPACE, LDS = 1, 2


@pytest.fixture(scope="module")
def ctx1():
    return true_rank_context()


def tens(v):
    import torch

    return torch.from_numpy(np.asarray(v, np.int32).reshape(-1).copy()).to("cuda:0")


@functools.lru_cache(maxsize=None)
def stream(k, m, nobj):
    from rlnc_amd import batch as rb

    return rb.DecodeStream(k, m, nobj, true_rank_context())


def staged(arrivals, base_off=0, pad=0, seed=1):
    """The arrivals in a staging buffer of random bytes, `base_off` bytes from a 16-byte boundary and `pad` bytes between
    rows: (the buffer, the strided [n][k + L] view of it)."""
    import torch

    n, S = arrivals.shape
    buf = dev(np.random.default_rng(seed).integers(0, 256, base_off + n * (S + pad) + 16, dtype=np.uint8))
    assert buf.data_ptr() % 16 == 0
    view = buf.as_strided((n, S), (S + pad, 1), base_off)
    view.copy_(torch.from_numpy(arrivals).to("cuda:0"))
    return buf, view


def accept_and_check(s, L, ids, avail, *, count=None, finished=None, base_off=0, pad=0, seed=0, tag="", pieces=None):
    """One accept on stream s over random arrivals and prefilled pieces; slot, avail, refused and every byte of the
    pieces against the model.  finished: the mask of the objects whose rank is k (the call passes the state), or None."""
    k, m, nobj = s.k, s.m, s.num_objects
    S, n = k + L, len(ids)
    rng = np.random.default_rng(1000 + seed)
    arrivals = rng.integers(0, 256, (n, S), dtype=np.uint8)
    p0 = rng.integers(0, 256, (nobj, m, S), dtype=np.uint8) if pieces is None else pieces
    _, view = staged(arrivals, base_off, pad, seed)
    assert view.data_ptr() % 16 == base_off % 16
    d_pieces, d_ids, d_avail = dev(p0), tens(ids), tens(avail)
    slot, refused = tens([-77] * n), tens([-77] * nobj)
    d_count = None if count is None else tens([count])
    s.accept(view, d_ids, d_pieces, d_avail, slot, refused, d_count, finished=finished is not None)
    want_slot, want_avail, want_refused = accept_model(ids, avail, m, nobj, count, finished)
    got_slot = host(slot)
    assert np.array_equal(got_slot, want_slot), (tag, np.flatnonzero(got_slot != want_slot)[:8], got_slot[:16], want_slot[:16])
    assert np.array_equal(host(d_avail), want_avail), (tag, host(d_avail)[:16], want_avail[:16])
    assert np.array_equal(host(refused), want_refused), (tag, host(refused)[:16], want_refused[:16])
    assert np.array_equal(host(d_pieces), place(p0, arrivals, ids, want_slot)), tag
    assert np.array_equal(host(d_ids), np.asarray(ids, np.int32)) and np.array_equal(host(view), arrivals), tag
    return want_slot


# ---- 1. piece widths -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", au.WIDTHS)
def test_piece_widths(S):
    """The byte path only, one partial lane, exactly one chunk, a tail folded into the last chunk, two chunks plus a
    tail: with the arrivals' base at byte offsets 0, 1 and 13 and the arrival stride at k + L and k + L + 3."""
    s = stream(1, au.WIDTH_M, au.WIDTH_OBJECTS)
    for base_off in (0, 1, 13):
        for pad in (0, 3):
            accept_and_check(s, S - 1, au.width_ids(), au.WIDTH_AVAIL, base_off=base_off, pad=pad, seed=S + base_off + pad,
                             tag=(S, base_off, pad))


# ---- 2. order --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(au.PATTERNS))
def test_order(name):
    k, L, m, nobj = au.ORDER_SHAPE
    accept_and_check(stream(k, m, nobj), L, pattern(name), [7, 9, 11] if name == "straddle" else [0, 5, m - 40],
                     seed=len(name), tag=name)


# ---- 3. clamps and codes ---------------------------------------------------------------------------------------------

def test_clamps_and_codes():
    ids, avail, m, nobj, _, _ = au.codes_case()
    n = len(ids)
    s = stream(3, m, nobj)
    for i, count in enumerate([None, 0, 1, n - 1, n, n + 5, -2]):
        slot = accept_and_check(s, 9, ids, avail, count=count, seed=i, tag=("count", count))
        assert (NO_OBJECT in slot) == (count is None or count > 2)
        assert (ABSENT in slot) == (count is not None and count < n)
    assert (slot == ABSENT).all()  # count -2: nothing is taken


# ---- 4. the finished filter ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [WORKSPACE, LDS], ids=["workspace", "lds"])
def test_finished_filter(form):
    from rlnc_amd import batch as rb

    k, m, L, nobj = 5, 7, 3, 4
    assert rb.stream_lds_fits(k, m)
    rng = np.random.default_rng(40)
    p0 = rng.integers(0, 256, (nobj, m, k + L), dtype=np.uint8)
    for o in (0, 2):
        p0[o, :k, :k] = independent(rng, k)
    pushed = [k, 2, k, 2]
    ctx = true_rank_context()
    ctx.set_stream_form(form)
    s = rb.DecodeStream(k, m, nobj, ctx)
    rank = tens([0] * nobj)
    s.push(dev(p0), tens(pushed), None, rank)
    assert host(rank).tolist() == [k, 2, k, 2]  # two objects are finished
    ids = np.array([0, 1, 2, 3, 0, 1, 2, 3, 1, 1, 1, 1, 3, 0, 7], np.int32)
    state = host(s.state).copy()
    slot = accept_and_check(s, L, ids, pushed, finished=[True, False, True, False], seed=1, tag="finished", pieces=p0)
    assert (slot[np.isin(ids, (0, 2))] == FINISHED).all() and (slot[ids == 1] == [2, 3, 4, 5, 6, NO_ROOM]).all()
    assert slot[ids == 3].tolist() == [2, 3, 4] and slot[-1] == NO_OBJECT
    slot = accept_and_check(s, L, ids, pushed, seed=1, tag="no state", pieces=p0)  # finished=False: all are placed
    assert FINISHED not in slot and slot[ids == 0].tolist() == [5, 6, NO_ROOM] and slot[ids == 2].tolist() == [5, 6]
    assert np.array_equal(host(s.state), state)


# ---- 5. footprint ----------------------------------------------------------------------------------------------------

def test_footprint():
    """Pieces (at an object stride beyond m(k+L), 3 bytes off a 16-byte boundary), avail, slot and refused in one arena
    with guards, prefilled from a seed: the assigned slots, the entries of avail but the finished object's, every entry
    of slot and refused change, to the model's values, and no other byte does; the arrivals, the ids, the count and the
    state are unchanged; the plan buffer's guards hold."""
    import torch

    from rlnc_amd import batch as rb

    k, m, L, nobj = 3, 5, 4110, 4
    S = k + L
    stride = m * S + 37
    ids = np.array([0, 1, 3, 2, 0, 9, 3, 2, 1, 0, 3, 3, 3, 0, 2], np.int32)
    n, count = len(ids), len(ids) - 2
    avail_in = np.array([-5, 3, m + 3, 2], np.int32)
    fin = [False, True, False, False]
    want_slot, want_avail, want_refused = accept_model(ids, avail_in, m, nobj, count, fin)
    assert {NO_ROOM, NO_OBJECT, FINISHED, ABSENT} <= set(want_slot.tolist()) and (want_slot >= 0).sum() >= 5
    assert all(want_avail[o] != avail_in[o] for o in (0, 2, 3)) and want_avail[1] == avail_in[1]
    rng = np.random.default_rng(50)
    arrivals = rng.integers(0, 256, (n, S), dtype=np.uint8)

    p_off = 3
    a_off = (p_off + nobj * stride + 15) // 16 * 16
    s_off = a_off + 16
    r_off = s_off + (4 * n + 15) // 16 * 16
    ar = Arena(r_off + 4 * nobj, seed=51, largest_row_stride=S)
    for i in np.flatnonzero(want_slot >= 0):
        ar.operand(f"piece of arrival {i}", p_off + int(ids[i]) * stride + int(want_slot[i]) * S, 1, 0, 1, S, S)
        ar.expect(f"piece of arrival {i}", arrivals[i])
    for o in range(nobj):
        if not fin[o]:
            ar.operand(f"avail[{o}]", a_off + 4 * o, 1, 0, 1, 4, 4)
            ar.expect(f"avail[{o}]", want_avail[o: o + 1])
    ar.operand("slot", s_off, 1, 0, n, 4, 4)
    ar.expect("slot", want_slot)
    ar.operand("refused", r_off, 1, 0, nobj, 4, 4)
    ar.expect("refused", want_refused)
    ar.seal()
    # the inputs that live in the arena, after the seal (avail is read and rewritten): avail, and the finished object's
    # pushed pieces
    ar.fill[ar.start + a_off: ar.start + a_off + 4 * nobj] = avail_in.view(np.uint8)
    ar.expected[ar.start + a_off + 4: ar.start + a_off + 8] = avail_in[1:2].view(np.uint8)
    obj1 = ar.start + p_off + stride
    ind = independent(rng, k)
    for t in range(k):
        ar.fill[obj1 + t * S: obj1 + t * S + k] = ar.expected[obj1 + t * S: obj1 + t * S + k] = ind[t]
    t = ar.device(seal=False)
    base = t.data_ptr() + ar.start
    assert base % 16 == 0
    d_pieces = ar.region()[p_off:].as_strided((nobj, m, S), (stride, S, 1))
    d_avail = ar.region()[a_off: a_off + 4 * nobj].view(torch.int32)

    s = rb.DecodeStream(k, m, nobj, true_rank_context())
    rank = tens([0] * nobj)
    s.push(d_pieces, tens([0, k, 0, 0]), None, rank)
    assert host(rank).tolist() == [0, k, 0, 0]
    state = host(s.state).copy()
    _, view = staged(arrivals, 5, 3)
    d_ids, d_count = tens(ids), tens([count])
    plan_bytes = rb.stream_accept_plan_bytes(n, nobj)
    qa = Arena(plan_bytes, seed=52)
    qa.device()
    ctx = s.ctx
    assert raw(ctx, "rlnc_decode_stream_accept", C.c_void_p(s.state.data_ptr()), s.state.numel(),
               C.c_void_p(view.data_ptr()), S + 3, C.c_void_p(d_ids.data_ptr()), n, C.c_void_p(d_count.data_ptr()),
               C.c_void_p(base + p_off), stride, k, L, m, nobj, C.c_void_p(base + a_off), C.c_void_p(base + s_off),
               C.c_void_p(base + r_off), C.c_void_p(qa.region().data_ptr()), plan_bytes) == 0, ctx.lib.rlnc_last_error()
    ar.check_device()
    assert host(d_avail).tolist() == want_avail.tolist()
    qa.check_guards(qa.after())
    assert np.array_equal(host(s.state), state), "the state changed"
    assert_inputs_unchanged({"arrivals": (arrivals, view), "object": (ids, d_ids),
                             "count": (np.array([count], np.int32), d_count)})


# ---- 6. equivalence with the host loop -------------------------------------------------------------------------------

def test_equivalence_with_the_host_loop():
    """Eight rounds of accept -> push -> deliver -> compact(retire, answered = avail) on one stream, and on a second one
    the slots filled by the host with filled[] kept there: after every round the live state of both, avail against
    filled and the delivered data are equal, and every object's decoded bytes are its source."""
    import torch

    from rlnc_amd import batch as rb

    k, m, L, nobj, rounds = 16, 20, 100, 6, 8
    S = k + L
    rng = np.random.default_rng(60)
    src = np.stack([npo.pad(rng.integers(0, 256, k * L - 1 - o, dtype=np.uint8), k) for o in range(nobj)])
    assert src.shape == (nobj, k, L)
    sent = [0] * nobj
    last = [None] * nobj

    def coded(o):
        """The object's next coded piece: a zero vector now and then, a duplicate of the one before now and then."""
        t = sent[o]
        sent[o] += 1
        if t % 7 == 3:
            co = np.zeros(k, np.uint8)
        elif t % 5 == 4:
            co = last[o]
        else:
            co = rng.integers(0, 256, k, dtype=np.uint8)
        last[o] = co
        return np.concatenate([co, np_matmul(co[None], src[o])[0]])

    dev_s, host_s = (rb.DecodeStream(k, m, nobj, true_rank_context()) for _ in range(2))
    fill = rng.integers(0, 256, (nobj, m, S), dtype=np.uint8)
    p_dev, p_host = dev(fill), dev(fill)
    avail = tens([0] * nobj)
    filled = [0] * nobj
    delivered = [False] * nobj
    outs = []
    for st in (dev_s, host_s):
        outs.append((torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0"), tens([-7] * nobj),
                     torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0"), tens([0] * nobj)))
    for rd in range(rounds):
        # three or four arrivals per object and round; a delivered object's place takes the same source again
        ids = np.array([o for o in range(nobj) for _ in range(3 + (rd + o) % 2)], np.int32)
        rng.shuffle(ids)
        arrivals = np.stack([coded(o) for o in ids])
        # on the device
        dec, ost, dl, retire = outs[0]
        dev_s.accept(dev(arrivals), tens(ids), p_dev, avail)
        dev_s.push(p_dev, avail)
        dev_s.deliver(p_dev, dec, ost, dl)
        retire.copy_((ost == 0).to(torch.int32))
        dev_s.compact(p_dev, retire, None, avail)
        # by the host
        dec2, ost2, dl2, retire2 = outs[1]
        d_arr = dev(arrivals)
        for i, o in enumerate(ids.tolist()):
            if filled[o] < m:
                p_host[o, filled[o]].copy_(d_arr[i])
                filled[o] += 1
        answered = tens([0] * nobj)
        host_s.push(p_host, tens(filled))
        host_s.deliver(p_host, dec2, ost2, dl2)
        retire2.copy_((ost2 == 0).to(torch.int32))
        host_s.compact(p_host, retire2, None, answered)
        filled = host(answered).tolist()
        # both
        assert host(avail).tolist() == filled, rd
        assert live_state(host(dev_s.state), k, m, nobj) == live_state(host(host_s.state), k, m, nobj), rd
        h_ost, h_dl, h_dec = host(ost), host(dl), host(dec)
        assert np.array_equal(h_ost, host(ost2)) and np.array_equal(h_dl, host(dl2)) and np.array_equal(h_dec, host(dec2))
        for o in range(nobj):
            if h_ost[o] == 0:
                delivered[o] = True
                assert h_dl[o] == k * L - 1 - o and np.array_equal(h_dec[o], src[o]), (rd, o)
                assert filled[o] == 0  # retired: its place is free
    assert all(delivered), delivered


# ---- 7. capture ------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch

k, m, L, nobj, n = 4, 12, 20, 3, 10
S = k + L
rng = np.random.default_rng(70)


def fresh():
    ctx = rlnc_amd.Context(0)
    ctx.set_rank_mode(1)
    return batch.DecodeStream(k, m, nobj, ctx)


def i32(v):
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device="cuda")


class Side:
    def __init__(self):
        self.s = fresh()
        self.pieces = torch.from_numpy(fill.copy()).cuda()
        self.arr = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
        self.ids, self.count, self.avail = i32([0] * n), i32([0]), i32([0] * nobj)
        self.slot, self.refused, self.rank, self.answered = i32([-7] * n), i32([-7] * nobj), i32([-7] * nobj), i32([-7] * nobj)

    def write(self, arr, ids, count, avail):
        self.arr.copy_(torch.from_numpy(arr))
        self.ids.copy_(torch.from_numpy(ids))
        self.count.fill_(count)
        if avail is not None:
            self.avail.copy_(torch.tensor(avail, dtype=torch.int32))
        torch.cuda.synchronize()

    def call(self):
        self.s.accept(self.arr, self.ids, self.pieces, self.avail, self.slot, self.refused, self.count, finished=True)
        self.s.push(self.pieces, self.avail, None, self.rank, self.answered)

    def image(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (self.pieces, self.avail, self.slot, self.refused, self.rank, self.answered)]


def round_inputs():
    return (rng.integers(0, 256, (n, S), dtype=np.uint8), rng.integers(-1, nobj + 1, n).astype(np.int32),
            int(rng.integers(-1, n + 3)))


fill = rng.integers(0, 256, (nobj, m, S), dtype=np.uint8)
cap, twin = Side(), Side()
first = round_inputs()
for side in (cap, twin):  # one eager round
    side.write(*first, [0] * nobj)
    side.call()
assert all(np.array_equal(a, b) for a, b in zip(cap.image(), twin.image()))
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap.call()
# the capture itself ran nothing: the twin does not move either
placed = 0
for rd in range(5):
    inputs = round_inputs()
    avail = [1, -3, m + 2] if rd == 2 else None  # a new avail now and then; otherwise the one the last round left
    cap.write(*inputs, avail)
    twin.write(*inputs, avail)
    g.replay()
    twin.call()
    a, b = cap.image(), twin.image()
    for x, y, name in zip(a, b, ("pieces", "avail", "slot", "refused", "rank", "answered")):
        assert np.array_equal(x, y), (rd, name, x, y)
    placed += int((a[2] >= 0).sum())
    assert (a[2][max(inputs[2], 0):] == -4).all()
assert placed >= 10, placed
print("stream accept graph ok")
"""


def test_accept_and_push_under_graph_capture():
    """In a fresh process: one eager round, then (accept, push) captured as one linear graph and replayed five times with
    new arrivals, ids, count and avail written into the same tensors: each replay equals the eager call on a twin."""
    code = CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream accept graph ok" in r.stdout


# ---- 8. scale --------------------------------------------------------------------------------------------------------

def test_scale_many_objects():
    """65,537 objects of (1, 2), two arrivals each, some of them for objects that are full by then."""
    nobj, m = 65537, 2
    rng = np.random.default_rng(80)
    ids = np.concatenate([np.arange(nobj), np.arange(nobj)]).astype(np.int32)
    rng.shuffle(ids)
    assert len(ids) == 131074
    avail = np.zeros(nobj, np.int32)
    avail[::1000] = 1  # the second arrival of these finds its object full
    avail[500::1000] = 2  # ... and both arrivals of these
    slot = accept_and_check(stream(1, m, nobj), 1, ids, avail, seed=80, tag="many objects")
    assert (slot == NO_ROOM).sum() == 66 + 2 * 66 and (slot >= 0).sum() > 130000


def test_scale_many_arrivals():
    """The most arrivals a call takes, 1,048,576, over 256 objects of m = 8,192: 1,024 dependent steps of the base launch;
    half the objects overflow."""
    nobj, m, n = 256, 8192, au.MAX_ARRIVALS
    rng = np.random.default_rng(81)
    ids = rng.integers(0, nobj, n).astype(np.int32)
    avail = np.where(np.arange(nobj) % 2 == 0, 0, m - 3000).astype(np.int32)
    slot = accept_and_check(stream(1, m, nobj), 1, ids, avail, seed=81, tag="many arrivals")
    assert (slot == NO_ROOM).sum() > 100000 and (slot >= 0).sum() > 800000


def test_far_object():
    """The last object's pieces lie more than 4 GiB from the base: the object stride is 2^32 + 4,097."""
    import torch

    k, m, L, nobj = 2, 4, 4111, 2
    S = k + L
    base = 8192 + 16 + 5
    torch.cuda.empty_cache()
    arena = FarArena(FAR_ODD + (1 << 26))
    try:
        ids = np.array([1, 0, 1, 1, 0, 1], np.int32)
        avail = [1, 2]
        want_slot, want_avail, want_refused = accept_model(ids, avail, m, nobj)
        assert want_slot.tolist() == [2, 1, 3, NO_ROOM, 2, NO_ROOM]
        arrivals = np.random.default_rng(82).integers(0, 256, (len(ids), S), dtype=np.uint8)
        lay = FarLayout(83, arena.size)
        for i in np.flatnonzero(want_slot >= 0):
            lay.write(f"piece of arrival {i}", base + int(ids[i]) * FAR_ODD + int(want_slot[i]) * S, 1, 0, 1, S, S, arrivals[i])
        lay.build()
        assert len(lay.windows) == 2 and lay.windows[1].lo - lay.windows[0].lo > 1 << 32
        pieces = arena.t.as_strided((nobj, m, S), (FAR_ODD, S, 1), base)
        d_avail, slot, refused = tens(avail), tens([-77] * len(ids)), tens([-77] * nobj)
        s = stream(k, m, nobj)
        arena.run(lay, lambda: s.accept(dev(arrivals), tens(ids), pieces, d_avail, slot, refused))
        assert host(slot).tolist() == want_slot.tolist() and host(d_avail).tolist() == want_avail.tolist()
        assert host(refused).tolist() == want_refused.tolist()
    finally:
        arena.t = None
        torch.cuda.empty_cache()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(ctx1):
    import rlnc_amd
    from rlnc_amd import batch as rb

    k, m, L, nobj, n = 11, 23, 50, 4, 9  # a shape no other test initialises: the library knows a state by its address
    S = k + L
    rng = np.random.default_rng(90)
    nbytes = rb.state_bytes(k, m, nobj)
    pb = rb.stream_accept_plan_bytes(n, nobj)
    buf = dev(rng.integers(0, 256, nbytes + 64, dtype=np.uint8))
    plan = dev(rng.integers(0, 256, pb + 64, dtype=np.uint8))
    pieces = dev(rng.integers(0, 256, (nobj, m, S), dtype=np.uint8))
    arrivals = dev(rng.integers(0, 256, (n, S), dtype=np.uint8))
    ids, avail, slot, refused = tens(rng.integers(0, nobj, n)), tens([1, 2, 3, 4]), tens([-77] * n), tens([-77] * nobj)
    assert buf.data_ptr() % 16 == 0 and plan.data_ptr() % 16 == 0
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def accept(ctx=ctx1, st=None, sn=nbytes, arr=ptr(arrivals), astride=0, ob=ptr(ids), n_=n, cnt=None, p=ptr(pieces),
               stride=0, k_=k, L_=L, m_=m, nobj_=nobj, av=ptr(avail), sl=ptr(slot), rf=ptr(refused), q=ptr(plan), qn=pb):
        return raw(ctx, "rlnc_decode_stream_accept", st, sn, arr, astride, ob, n_, cnt, p, stride, k_, L_, m_, nobj_, av,
                   sl, rf, q, qn)

    every = (buf, plan, pieces, arrivals, ids, avail, slot, refused)
    held = [host(t).copy() for t in every]

    def untouched():
        return all(np.array_equal(host(t), h) for t, h in zip(every, held))

    err = ctx1.lib.rlnc_last_error
    state = ptr(buf)
    assert accept(st=state) == INVALID and b"not initialised" in err() and untouched()  # a state never initialised
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
    held[0] = host(buf).copy()
    ctx0 = rlnc_amd.Context(0)
    assert accept(ctx=ctx0, st=state) == INVALID and b"rank mode" in err()  # a rank-mode-0 context, with a state
    # a state initialised for another shape, short, misaligned
    assert accept(st=state, k_=k - 1) == INVALID and accept(st=state, m_=m - 1) == INVALID
    assert accept(st=state, nobj_=nobj - 1) == INVALID and b"not initialised" in err()
    assert accept(st=state, sn=nbytes - 16) == INVALID and accept(st=C.c_void_p(buf.data_ptr() + 4)) == INVALID
    # the shape, even without a state
    assert accept(m_=0) == INVALID and b"8192" in err() and accept(m_=8193, stride=2 ** 40) == INVALID and b"8192" in err()
    assert accept(k_=4097) == INVALID and b"4096" in err()
    assert accept(n_=au.MAX_ARRIVALS + 1, qn=2 ** 40) == INVALID and b"1048576" in err()
    assert accept(astride=S - 1) == INVALID and b"arrival_stride" in err()
    assert accept(stride=m * S - 1) == INVALID and b"obj_stride" in err()
    assert accept(arr=None) == INVALID and accept(ob=None) == INVALID and accept(p=None) == INVALID
    assert accept(av=None) == INVALID
    assert accept(q=None) == INVALID and b"plan" in err()
    assert accept(q=C.c_void_p(plan.data_ptr() + 8)) == INVALID and b"plan" in err()
    assert accept(qn=pb - 16) == INVALID and b"plan" in err() and str(pb).encode() in err()
    assert accept(qn=rb.stream_accept_plan_bytes(n - 5, nobj)) == INVALID and b"plan" in err()  # sized for fewer arrivals
    assert accept(n_=au.MAX_ARRIVALS, L_=4096 * 2048, qn=2 ** 40) == INVALID and b"workgroups" in err()
    # the crate's checks come first, in push's order; no arrivals or no objects: nothing to do
    assert accept(k_=0, L_=0) == 3 and accept(L_=0) == 5
    assert accept(n_=0, q=None) == 0 and accept(nobj_=0, q=None) == 0
    assert untouched()
    # and the call works: without a state, with one, with slot and refused left out
    want_slot, want_avail, want_refused = accept_model(held[4], held[5], m, nobj)
    assert accept(sl=None, rf=None) == 0
    assert np.array_equal(host(avail), want_avail) and np.array_equal(host(slot), held[6])
    assert np.array_equal(host(refused), held[7])
    assert np.array_equal(host(pieces), place(held[2], held[3], held[4], want_slot))
    avail.copy_(tens(held[5]))
    assert accept(st=state) == 0
    assert np.array_equal(host(slot), want_slot) and np.array_equal(host(refused), want_refused)
    assert np.array_equal(host(avail), want_avail) and np.array_equal(host(buf), held[0])
