"""GPU: a decode stream's recode (include/rlnc_hip.h, rlnc_decode_stream_recode; rlnc_amd/csrc/stream_recode.hip;
rlnc_amd.batch.DecodeStream.recode) on the batches of tests/recode_util.py, whose objects
tests/test_decode_stream_recode_host.py holds to their names.  All comparisons are exact.

A recode must hand every selected object of rank r > 0 count combinations of exactly its useful pieces, header and data
alike, with status Ok and used = r; an object of rank 0 gets NotEnoughPiecesToRecode, used 0 and no byte of out; an
unselected object gets nothing at all; the state, the pieces, r and select are only read."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.deliver_util import independent
from tests.footprint import Arena
from tests.gpu_util import dev, host, np_matmul
from tests.recode_util import FULL, NAMES, NOT_ENOUGH, REFUSAL_SHAPE, SHAPES, batch, expected_of
from tests.stream_util import raw, true_rank_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 100
WORKSPACE, LDS = 1, 2
NOBJ = len(NAMES)


@pytest.fixture(scope="module")
def ctx1():
    return true_rank_context()


def tens(v):
    import torch

    return torch.tensor([int(x) for x in v], dtype=torch.int32, device="cuda:0")


class Outputs:
    """out, status and used prefilled from a seed, with the host copy of the prefill."""

    def __init__(self, k, L, count, seed, nobj=NOBJ):
        import torch

        rng = np.random.default_rng(seed)
        self.fill = (rng.integers(0, 256, (nobj, count, k + L), dtype=np.uint8),
                     rng.integers(-2 ** 31, -1, nobj, dtype=np.int32),
                     rng.integers(-2 ** 31, -1, nobj, dtype=np.int32))
        self.out, self.status, self.used = (torch.from_numpy(a.copy()).to("cuda:0") for a in self.fill)

    def args(self):
        return self.out, self.status, self.used

    def host(self):
        return host(self.out), host(self.status), host(self.used)


def pushed(ctx, b, pieces=None):
    from rlnc_amd import batch as rb

    s = rb.DecodeStream(b.k, b.m, NOBJ, ctx)
    p = dev(b.pieces.copy()) if pieces is None else pieces
    s.push(p, tens(b.done))
    return s, p


@functools.lru_cache(maxsize=None)
def reference(k, m, L, count):
    """Per shape, once: a pushed stream, its pieces and r on the device, and what a recode of every object answers."""
    b = batch(k, m, L, count)
    s, p = pushed(true_rank_context(), b)
    r = dev(b.r.copy())
    rc = Outputs(k, L, count, seed=12)
    s.recode(p, r, *rc.args())
    got = rc.host()
    for t in got:
        t.setflags(write=False)
    return s, p, r, got, rc.fill


def check_recode(b, got, fill, selected, tag, expected=None):
    """got = (out, status, used) after a recode of the objects in `selected` over the prefill `fill`."""
    out, st, us = got
    expected = b.expected if expected is None else expected
    for o, name in enumerate(NAMES):
        if o not in selected:
            assert np.array_equal(out[o], fill[0][o]) and st[o] == fill[1][o] and us[o] == fill[2][o], (tag, name)
            continue
        assert st[o] == b.status[o] and us[o] == b.rank[o], (tag, name, st[o], us[o])
        if b.rank[o] == 0:
            assert st[o] == NOT_ENOUGH and np.array_equal(out[o], fill[0][o]), (tag, name)
        else:
            assert st[o] == 0 and np.array_equal(out[o], expected[o]), (tag, name)


# ---- 1. bytes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L,count", SHAPES)
def test_recodes_over_the_useful_pieces(k, m, L, count):
    import torch

    from rlnc_amd import batch as rb

    b = batch(k, m, L, count)
    _, _, _, got, fill = reference(k, m, L, count)
    check_recode(b, got, fill, set(range(NOBJ)), "all")
    for o, name in enumerate(NAMES):  # the header part is r x co[u]
        if b.rank[o]:
            u = list(b.useful[o])
            assert np.array_equal(got[0][o][:, :k], np_matmul(b.r[o][:, : b.rank[o]], b.co[o][u])), name
    # ... and `padded` agrees with the existing recode over the pieces gathered by the host
    o = NAMES.index("padded")
    u = list(b.useful[o])
    gathered = dev(b.pieces[o][u][None])
    ro = dev(b.r[o][None, :, : b.rank[o]].copy())
    out = torch.zeros((1, count, k + L), dtype=torch.uint8, device="cuda:0")
    rb.recode_batch(gathered, ro, out, k)
    assert np.array_equal(host(out)[0], got[0][o])


# ---- 2. select -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L,count", SHAPES)
def test_select(k, m, L, count):
    b = batch(k, m, L, count)
    s, p, r, _, _ = reference(k, m, L, count)
    masks = {"none": [0] * NOBJ, "every second": [o % 2 for o in range(NOBJ)],
             "rank 0 only": [int(x == 0) for x in b.rank]}
    assert sum(masks["rank 0 only"]) >= 2
    for i, (tag, mask) in enumerate(masks.items()):
        out = Outputs(k, L, count, seed=20 + i)
        sel = tens([7 * x for x in mask])  # any nonzero value selects
        s.recode(p, r, *out.args(), select=sel)
        check_recode(b, out.host(), out.fill, {o for o in range(NOBJ) if mask[o]}, tag)
        assert host(sel).tolist() == [7 * x for x in mask]


# ---- 3. footprint ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L,count", [(3, 5, 4099, 3), (16, 20, 4099, 16), (16, 24, 4100, 70)])
def test_footprint(ctx1, k, m, L, count):
    """Every buffer in an arena with guards, prefilled from a seed.  The state, the pieces (at an object stride larger
    than m(k+L), the pad included), r and select are byte-identical after the call; of out only the count x (k+L) bytes
    of the recoding objects change, of status and used only the selected entries; the plan buffer's guards hold."""
    from rlnc_amd import batch as rb

    b = batch(k, m, L, count)
    S = k + L
    nbytes = rb.state_bytes(k, m, NOBJ)
    sa = Arena(nbytes, seed=600)
    sa.device()
    state = C.c_void_p(sa.region().data_ptr())
    stride = m * S + 37
    pa = Arena(NOBJ * stride, seed=601, base_off=5, largest_row_stride=S)
    pa.fill[pa.start: pa.end].reshape(NOBJ, stride)[:, : m * S] = b.pieces.reshape(NOBJ, -1)
    pa.expected[:] = pa.fill
    pa.device()
    pieces = C.c_void_p(pa.region().data_ptr())
    ra = Arena(NOBJ * count * k, seed=605, base_off=7)
    ra.fill[ra.start: ra.end] = b.r.reshape(-1)
    ra.expected[:] = ra.fill
    ra.device()
    mask = [1] * NOBJ
    mask[NAMES.index("over")] = mask[NAMES.index("empty")] = 0  # one that would recode and one of rank 0 go unselected
    la = Arena(NOBJ * 4, seed=602)
    la.fill[la.start: la.end] = np.array(mask, np.int32).view(np.uint8)
    la.expected[:] = la.fill
    la.device()
    plan_bytes = rb.stream_recode_plan_bytes(k, m, count, NOBJ)
    qa = Arena(plan_bytes, seed=603)
    qa.device()
    oa = Arena(NOBJ * count * S + 160, seed=604, base_off=3, largest_row_stride=S)
    st_off = (NOBJ * count * S + 3 + 15) // 16 * 16 - 3  # status and used aligned as int32 needs
    us_off = st_off + NOBJ * 4
    for o, name in enumerate(NAMES):
        if not mask[o]:
            continue
        if b.rank[o]:
            oa.operand(f"out[{name}]", o * count * S, 1, 0, count, S, S)
            oa.expect(f"out[{name}]", b.expected[o])
        oa.operand(f"status[{name}]", st_off + 4 * o, 1, 0, 1, 4, 4)
        oa.expect(f"status[{name}]", np.array([b.status[o]], np.int32))
        oa.operand(f"used[{name}]", us_off + 4 * o, 1, 0, 1, 4, 4)
        oa.expect(f"used[{name}]", np.array([b.rank[o]], np.int32))
    oa.device()
    base = oa.region().data_ptr()
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, NOBJ) == 0
    av = tens(b.done)
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, pieces, stride, k, L, m, NOBJ, C.c_void_p(av.data_ptr()),
               m, None, None) == 0
    before = sa.after().copy()
    assert raw(ctx1, "rlnc_decode_stream_recode", state, nbytes, pieces, stride, k, L, m, NOBJ,
               C.c_void_p(la.region().data_ptr()), C.c_void_p(ra.region().data_ptr()), count, C.c_void_p(base),
               C.c_void_p(base + st_off), C.c_void_p(base + us_off), C.c_void_p(qa.region().data_ptr()),
               plan_bytes) == 0, ctx1.lib.rlnc_last_error()
    oa.check_device()
    assert np.array_equal(sa.after(), before), "the state changed"
    pa.check_device()
    ra.check_device()
    la.check_device()
    qa.check_guards(qa.after())


# ---- 4. after a compaction -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L,count", SHAPES)
def test_after_a_compaction(k, m, L, count):
    """The kept pieces are the useful ones, so the same r gives the same bytes, and used is unchanged."""
    b = batch(k, m, L, count)
    _, _, r, ref, _ = reference(k, m, L, count)
    s, p = pushed(true_rank_context(), b)
    ans = tens([0] * NOBJ)
    s.compact(p, None, None, ans)
    assert host(ans).tolist() == list(b.rank)  # done = rank now: the minimal product
    out = Outputs(k, L, count, seed=12)  # reference()'s prefill
    s.recode(p, r, *out.args())
    got = out.host()
    check_recode(b, got, out.fill, set(range(NOBJ)), "compacted")
    for x, y in zip(got, ref):
        assert np.array_equal(x, y)


# ---- 5. both push forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L,count", [(16, 20, 4099, 16), (40, 48, 4096, 40)])
def test_both_push_forms(k, m, L, count):
    from rlnc_amd import batch as rb

    assert rb.stream_lds_fits(k, m)
    b = batch(k, m, L, count)
    _, _, r, ref, _ = reference(k, m, L, count)
    for form in (WORKSPACE, LDS):
        ctx = true_rank_context()
        ctx.set_stream_form(form)
        s, p = pushed(ctx, b)
        out = Outputs(k, L, count, seed=12)  # reference()'s prefill
        s.recode(p, r, *out.args())
        got = out.host()
        check_recode(b, got, out.fill, set(range(NOBJ)), form)
        for x, y in zip(got, ref):
            assert np.array_equal(x, y), form


# ---- 6. a relay, end to end ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L,count", [(3, 5, 4099, 3), (16, 20, 4099, 16), (40, 48, 4096, 40)])
def test_a_relay_forwards_what_a_receiver_decodes(ctx1, k, m, L, count):
    """count = k and an invertible r: the recoded pieces of the rank-k objects, pushed to a second stream, reach rank k
    there, and its delivery is the original source and length."""
    import torch

    from rlnc_amd import batch as rb

    assert count == k
    b = batch(k, m, L, count)
    s, p, _, _, _ = reference(k, m, L, count)
    rng = np.random.default_rng(90 + k)
    r = np.stack([independent(rng, k) for _ in range(NOBJ)])
    out = Outputs(k, L, k, seed=91)
    s.recode(p, dev(r), *out.args())
    got = out.host()
    check_recode(b, got, out.fill, set(range(NOBJ)), "relay", [expected_of(b, o, r[o]) for o in range(NOBJ)])
    full = [o for o, name in enumerate(NAMES) if name in FULL]
    assert all(b.rank[o] == k for o in full)
    relayed = out.out[full].contiguous()  # [4][k][k + L]: on the device throughout
    s2 = rb.DecodeStream(k, k, len(full), ctx1)
    rank = tens([0] * len(full))
    s2.push(relayed, tens([k] * len(full)), None, rank)
    assert host(rank).tolist() == [k] * len(full)
    decoded = torch.zeros((len(full), k, L), dtype=torch.uint8, device="cuda:0")
    ost = tens([-7] * len(full))
    dl = torch.full((len(full),), -1, dtype=torch.int64, device="cuda:0")
    s2.deliver(relayed, decoded, ost, dl)
    assert host(ost).tolist() == [0] * len(full)
    assert host(dl).tolist() == [b.data_len[o] for o in full]
    assert np.array_equal(host(decoded), b.src[full])


# ---- 7. capture ------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch
from tests.gpu_util import np_matmul

k, m, L, nobj, count = 24, 30, 4113, 3, 24  # the 4-wave shared program: its block-table probe cannot run in a capture
rng = np.random.default_rng(80)
src = rng.integers(0, 256, (nobj, k, L), dtype=np.uint8)
co = rng.integers(1, 256, (nobj, m, k), dtype=np.uint8)
co[:, 2] = 0  # a useless slot: done > rank
p = np.stack([np.concatenate([co[o], np_matmul(co[o], src[o])], axis=1) for o in range(nobj)])
pieces = torch.from_numpy(p).cuda()


def expect(done, r, prev):
    # slot 2 is useless and the others independent: rank k is reached with slot k, later slots are ReceivedAllPieces
    out, st, us = prev.copy(), [], []
    for o in range(nobj):
        u = [t for t in range(done[o]) if t != 2][:k]
        st.append(0 if u else 6)
        us.append(len(u))
        if u:
            out[o] = np_matmul(r[o][:, : len(u)], p[o][u])
    return out, st, us


def fresh():
    ctx = rlnc_amd.Context(0)
    ctx.set_rank_mode(1)
    return batch.DecodeStream(k, m, nobj, ctx)


out = torch.zeros((nobj, count, k + L), dtype=torch.uint8, device="cuda")
ost = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
used = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
avail = torch.zeros(nobj, dtype=torch.int32, device="cuda")
r_h = rng.integers(0, 256, (nobj, count, k), dtype=np.uint8)
r = torch.from_numpy(r_h).cuda()

# ---- a first recode inside a capture: no block table yet, the tail kernel takes every column -- the same bytes
first = fresh()
avail.copy_(torch.tensor([9, 0, 30], dtype=torch.int32))
first.push(pieces, avail)
first.recode_reserve(count)
torch.cuda.synchronize()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s):
        first.recode(pieces, r, out, ost, used)
g0.replay()
torch.cuda.synchronize()
want, st, us = expect([9, 0, 30], r_h, np.zeros((nobj, count, k + L), np.uint8))
assert ost.cpu().tolist() == st == [0, 6, 0] and used.cpu().tolist() == us == [8, 0, k], (ost, used)
assert np.array_equal(out.cpu().numpy(), want)
tail_bytes, r_first = out.cpu().numpy().copy(), r_h.copy()

# ---- one eager push and one eager recode, then (push, recode) captured and replayed while avail and r change
cap = fresh()
out.zero_()
avail.copy_(torch.tensor([3, 0, 1], dtype=torch.int32))
cap.push(pieces, avail, 8)
cap.recode(pieces, r, out, ost, used)
torch.cuda.synchronize()
done = [3, 0, 1]
prev, st, us = expect(done, r_h, np.zeros((nobj, count, k + L), np.uint8))
assert ost.cpu().tolist() == st == [0, 6, 0] and used.cpu().tolist() == us == [2, 0, 1]
assert np.array_equal(out.cpu().numpy(), prev)
with torch.cuda.stream(s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap.push(pieces, avail, 8)
        cap.recode(pieces, r, out, ost, used)
rounds = [[5, 9, 1], [12, 9, 20], [20, 26, 20], [30, 26, 24], [30, 26, 30], [30, 30, 30]]
for rd in rounds:
    avail.copy_(torch.tensor(rd, dtype=torch.int32))
    r_h = rng.integers(0, 256, (nobj, count, k), dtype=np.uint8)
    r.copy_(torch.from_numpy(r_h))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    done = [min(max(a, d), m, d + 8) for d, a in zip(done, rd)]
    prev, st, us = expect(done, r_h, prev)
    assert ost.cpu().tolist() == st and used.cpu().tolist() == us, (rd, ost, used, st, us)
    assert np.array_equal(out.cpu().numpy(), prev), rd
assert used.cpu().tolist() == [k] * nobj

# ---- and the eager program's bytes are the captured tail kernel's
out.zero_()
first.recode(pieces, torch.from_numpy(r_first).cuda(), out, ost, used)
torch.cuda.synchronize()
assert np.array_equal(out.cpu().numpy(), tail_bytes) and used.cpu().tolist() == [8, 0, k]
print("stream recode graph ok")
"""


def test_push_and_recode_under_graph_capture():
    """In a fresh process: a first recode inside a capture (no block table yet) gives the model's bytes through the tail
    kernel; then, after one eager recode, (push, recode) captured as one linear graph and replayed over the rounds while
    avail and the bytes of r change: the outputs follow."""
    code = CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream recode graph ok" in r.stdout


# ---- 8. errors -------------------------------------------------------------------------------------------------------

def test_refusals(ctx1):
    import rlnc_amd
    from rlnc_amd import batch as rb

    k, m, L, count = REFUSAL_SHAPE  # a shape no other test initialises: the library knows a state by its address
    b = batch(k, m, L, count)
    nbytes = rb.state_bytes(k, m, NOBJ)
    pb = rb.stream_recode_plan_bytes(k, m, count, NOBJ)
    buf = dev(np.random.default_rng(60).integers(0, 256, nbytes + 64, dtype=np.uint8))
    plan = dev(np.random.default_rng(61).integers(0, 256, pb + 64, dtype=np.uint8))
    pieces = dev(b.pieces.copy())
    r = dev(b.r.copy())
    out = Outputs(k, L, count, seed=62)
    assert buf.data_ptr() % 16 == 0 and plan.data_ptr() % 16 == 0
    state, pp, qp, rp = (C.c_void_p(t.data_ptr()) for t in (buf, pieces, plan, r))
    op, sp, up = (C.c_void_p(t.data_ptr()) for t in out.args())

    def recode(ctx=ctx1, st=state, n=nbytes, p=pp, stride=0, k_=k, L_=L, m_=m, nobj=NOBJ, r_=rp, c=count, o=op, s=sp, u=up,
               q=qp, qn=pb):
        return raw(ctx, "rlnc_decode_stream_recode", st, n, p, stride, k_, L_, m_, nobj, None, r_, c, o, s, u, q, qn)

    every = (buf, plan, pieces, r) + out.args()
    held = [host(t).copy() for t in every]

    def untouched():
        return all(np.array_equal(host(t), h) for t, h in zip(every, held))

    err = ctx1.lib.rlnc_last_error
    assert recode() == INVALID and b"not initialised" in err() and untouched()  # a state never initialised
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, NOBJ) == 0
    av = tens(b.done)
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, pp, 0, k, L, m, NOBJ, C.c_void_p(av.data_ptr()), m, None,
               None) == 0
    held[0] = host(buf).copy()
    ctx0 = rlnc_amd.Context(0)
    assert recode(ctx=ctx0) == INVALID and b"rank mode" in err()  # a rank-mode-0 context
    # a state initialised for another shape
    assert recode(k_=k - 1) == INVALID and recode(m_=m - 1) == INVALID and recode(nobj=NOBJ - 1) == INVALID
    assert b"not initialised" in err()
    assert recode(n=nbytes - 16) == INVALID and recode(st=C.c_void_p(buf.data_ptr() + 4)) == INVALID
    assert recode(st=None) == INVALID
    assert recode(qn=pb - 16) == INVALID and b"plan" in err() and str(pb).encode() in err()  # a short plan buffer
    assert recode(q=C.c_void_p(plan.data_ptr() + 8)) == INVALID and b"plan" in err()  # a misaligned one
    assert recode(q=None) == INVALID and b"plan" in err()
    # a plan sized for a smaller count
    assert recode(qn=rb.stream_recode_plan_bytes(k, m, count - 1, NOBJ)) == INVALID and b"plan" in err()
    assert recode(stride=m * (k + L) - 1) == INVALID and b"obj_stride" in err()  # a stride below m(k+L)
    assert recode(p=None) == INVALID and recode(o=None) == INVALID and recode(r_=None) == INVALID
    assert recode(s=None) == INVALID
    assert recode(c=4097, qn=2 ** 40) == INVALID and b"4096" in err()  # more than a call recodes
    # the crate's checks come first, in push's order; no objects or no pieces to make: nothing to do
    assert recode(k_=0, L_=0, st=None) == 3 and recode(L_=0, st=None) == 5
    assert recode(nobj=0, st=None) == 0 and recode(c=0, st=None) == 0
    assert untouched()
    # and the call works, used being optional
    assert recode(u=None) == 0
    got = out.host()
    assert np.array_equal(got[2], out.fill[2])
    check_recode(b, (got[0], got[1], np.array(b.rank, np.int32)), out.fill, set(range(NOBJ)), "works")
    assert np.array_equal(host(buf), held[0]) and np.array_equal(host(pieces), held[2])
