"""GPU: a decode stream's delivery (include/rlnc_hip.h, rlnc_decode_stream_deliver; rlnc_amd/csrc/stream_deliver.hip;
rlnc_amd.batch.DecodeStream.deliver) on the batches of tests/deliver_util.py, whose objects
tests/test_decode_stream_deliver_host.py holds to their names.  All comparisons are exact.

A delivery must hand over the source rows of every object of rank k and its status and length exactly as
DecodeStream.apply (snapshot + rlnc_decode_batch_apply, existing code) answers them from the same state; it must write no
byte of an object below rank k but its status and length, nothing at all of an unselected object, and nothing of the
state, the pieces or select."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.deliver_util import FULL, NAMES, NOT_ALL, REFUSAL_SHAPE, SHAPES, batch
from tests.footprint import Arena
from tests.gpu_util import dev, host, np_matmul
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
    """decoded, object_status and data_len prefilled from a seed, with the host copy of the prefill."""

    def __init__(self, k, L, seed, nobj=NOBJ):
        import torch

        rng = np.random.default_rng(seed)
        self.fill = (rng.integers(0, 256, (nobj, k, L), dtype=np.uint8),
                     rng.integers(-2 ** 31, 2 ** 31, nobj, dtype=np.int32),
                     rng.integers(-2 ** 62, 2 ** 62, nobj, dtype=np.int64))
        self.decoded, self.status, self.length = (torch.from_numpy(a.copy()).to("cuda:0") for a in self.fill)

    def args(self):
        return self.decoded, self.status, self.length

    def host(self):
        return host(self.decoded), host(self.status), host(self.length)


def pushed(ctx, b, pieces=None):
    from rlnc_amd import batch as rb

    s = rb.DecodeStream(b.k, b.m, NOBJ, ctx)
    p = dev(b.pieces.copy()) if pieces is None else pieces
    s.push(p, tens(b.done))
    return s, p


@functools.lru_cache(maxsize=None)
def reference(k, m, L):
    """Per shape, once: a pushed stream, its pieces on the device, what DecodeStream.apply answers from that state
    (decoded, statuses, lengths: existing code, buffers of its own) and what a delivery of every object answers."""
    b = batch(k, m, L)
    ctx = true_rank_context()
    s, p = pushed(ctx, b)
    ap = Outputs(k, L, seed=11)
    s.apply(p, *ap.args())
    dl = Outputs(k, L, seed=12)
    s.deliver(p, *dl.args())
    out = (s, p, ap.host(), dl.host(), dl.fill)
    for t in out[2] + out[3]:
        t.setflags(write=False)
    return out


def check_delivery(b, got, fill, apply_out, selected, tag):
    """got = (decoded, status, length) after a delivery of the objects in `selected` over the prefill `fill`."""
    dec, st, ln = got
    a_dec, a_st, a_ln = apply_out
    for o, name in enumerate(NAMES):
        if o not in selected:
            assert np.array_equal(dec[o], fill[0][o]) and st[o] == fill[1][o] and ln[o] == fill[2][o], (tag, name)
            continue
        assert st[o] == a_st[o] == b.status[o] and ln[o] == a_ln[o] == b.length[o], (tag, name, st[o], ln[o])
        if name in FULL:
            assert np.array_equal(dec[o], b.src[o]), (tag, name)
            assert np.array_equal(dec[o], a_dec[o]), (tag, name)
        else:
            assert st[o] == NOT_ALL and ln[o] == 0 and np.array_equal(dec[o], fill[0][o]), (tag, name)


# ---- 1. against the source and against apply -------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L", SHAPES)
def test_delivers_the_source_and_answers_as_apply(k, m, L):
    b = batch(k, m, L)
    _, _, ap, got, fill = reference(k, m, L)
    check_delivery(b, got, fill, ap, set(range(NOBJ)), "all")
    assert np.array_equal(got[1], ap[1]) and np.array_equal(got[2], ap[2])


# ---- 2. select -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L", SHAPES)
def test_select(k, m, L):
    b = batch(k, m, L)
    s, p, ap, _, _ = reference(k, m, L)
    masks = {"none": [0] * NOBJ, "every second": [o % 2 for o in range(NOBJ)],
             "below rank k": [int(n not in FULL) for n in NAMES]}
    for i, (tag, mask) in enumerate(masks.items()):
        out = Outputs(k, L, seed=20 + i)
        sel = tens([7 * x for x in mask])  # any nonzero value selects
        s.deliver(p, *out.args(), select=sel)
        check_delivery(b, out.host(), out.fill, ap, {o for o in range(NOBJ) if mask[o]}, tag)
        assert host(sel).tolist() == [7 * x for x in mask]


# ---- 3. after a compaction; the state is untouched -------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L", SHAPES)
def test_after_a_compaction(k, m, L):
    b = batch(k, m, L)
    _, _, ap, _, _ = reference(k, m, L)
    s, p = pushed(true_rank_context(), b)
    ans = tens([0] * NOBJ)
    s.compact(p, None, None, ans)
    # done = rank now: the minimal product
    assert all(a == k for n, a in zip(NAMES, host(ans).tolist()) if n in FULL)
    out = Outputs(k, L, seed=30)
    s.deliver(p, *out.args())
    check_delivery(b, out.host(), out.fill, ap, set(range(NOBJ)), "compacted")


@pytest.mark.parametrize("k,m,L", SHAPES)
def test_a_delivery_leaves_the_stream_as_it_was(k, m, L):
    """deliver, a push of extra arrivals, deliver: the objects of rank k answer the same bytes again, and an object the
    new arrivals complete is delivered too -- the first delivery changed nothing a push reads."""
    b = batch(k, m, L)
    _, _, ap, _, _ = reference(k, m, L)
    s, p = pushed(true_rank_context(), b)
    image = host(s.state).copy()
    out = Outputs(k, L, seed=40)
    s.deliver(p, *out.args())
    check_delivery(b, out.host(), out.fill, ap, set(range(NOBJ)), "first")
    assert np.array_equal(host(s.state), image)
    rng = np.random.default_rng(41)
    avail = list(b.done)
    for o in range(NOBJ):
        n = min(2, m - b.done[o])
        co = rng.integers(1, 256, (n, k), dtype=np.uint8)
        if n:
            p[o, b.done[o]: b.done[o] + n] = dev(np.concatenate([co, np_matmul(co, b.src[o])], axis=1))
        avail[o] += n
    rank = tens([0] * NOBJ)
    s.push(p, tens(avail), None, rank)
    out2 = Outputs(k, L, seed=42)
    s.deliver(p, *out2.args())
    dec, st, ln = out2.host()
    rank = host(rank).tolist()
    for o, name in enumerate(NAMES):
        if name in FULL:
            assert rank[o] == k and np.array_equal(dec[o], b.src[o]) and (st[o], ln[o]) == (b.status[o], b.length[o]), name
        elif rank[o] == k:
            assert np.array_equal(dec[o], b.src[o]) and (st[o], ln[o]) == (0, b.data_len[o]), name
        else:
            assert st[o] == NOT_ALL and ln[o] == 0 and np.array_equal(dec[o], out2.fill[0][o]), name
    if k >= 2:  # one more independent vector completes `short`
        assert rank[NAMES.index("short")] == k


# ---- 4. both push forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L", [(16, 20, 4099), (70, 80, 4100)])  # inside / outside the automatic LDS rule
def test_both_push_forms(k, m, L):
    from rlnc_amd import batch as rb

    assert rb.stream_lds_fits(k, m) and ((k <= 48 and m <= 64) == (k == 16))
    b = batch(k, m, L)
    _, _, ap, ref, _ = reference(k, m, L)
    for form in (WORKSPACE, LDS):
        ctx = true_rank_context()
        ctx.set_stream_form(form)
        s, p = pushed(ctx, b)
        out = Outputs(k, L, seed=12)  # reference()'s prefill
        s.deliver(p, *out.args())
        got = out.host()
        check_delivery(b, got, out.fill, ap, set(range(NOBJ)), form)
        for x, y in zip(got, ref):
            assert np.array_equal(x, y), form


# ---- 5. footprint ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,L", [(3, 5, 4099), (16, 20, 4099), (70, 80, 4100)])
def test_footprint(ctx1, k, m, L):
    """Every buffer in an arena with guards, prefilled from a seed.  The state, the pieces (at an object stride larger
    than m(k+L), the pad included) and select are byte-identical after the call; of decoded only the k x L bytes of the
    delivering objects change, of status and length only the selected entries; the plan buffer's guards hold."""
    from rlnc_amd import batch as rb

    b = batch(k, m, L)
    nbytes = rb.state_bytes(k, m, NOBJ)
    sa = Arena(nbytes, seed=500)
    sa.device()
    state = C.c_void_p(sa.region().data_ptr())
    stride = m * (k + L) + 37
    pa = Arena(NOBJ * stride, seed=501, base_off=5, largest_row_stride=k + L)
    pa.fill[pa.start: pa.end].reshape(NOBJ, stride)[:, : m * (k + L)] = b.pieces.reshape(NOBJ, -1)
    pa.expected[:] = pa.fill
    pa.device()
    pieces = C.c_void_p(pa.region().data_ptr())
    mask = [1] * NOBJ
    mask[NAMES.index("over")] = mask[NAMES.index("deficient")] = 0  # one of rank k and one below it go unselected
    la = Arena(NOBJ * 4, seed=502)
    la.fill[la.start: la.end] = np.array(mask, np.int32).view(np.uint8)
    la.expected[:] = la.fill
    la.device()
    plan_bytes = rb.stream_deliver_plan_bytes(k, m, NOBJ)
    qa = Arena(plan_bytes, seed=503)
    qa.device()
    oa = Arena(NOBJ * k * L + 160, seed=504, base_off=3, largest_row_stride=L)
    st_off = (NOBJ * k * L + 3 + 15) // 16 * 16 - 3  # status and length aligned as int32 / int64 need
    ln_off = st_off + (NOBJ * 4 + 7) // 8 * 8
    for o, name in enumerate(NAMES):
        if not mask[o]:
            continue
        if name in FULL:
            oa.operand(f"decoded[{name}]", o * k * L, 1, 0, k, L, L)
            oa.expect(f"decoded[{name}]", b.src[o])
        oa.operand(f"status[{name}]", st_off + 4 * o, 1, 0, 1, 4, 4)
        oa.expect(f"status[{name}]", np.array([b.status[o]], np.int32))
        oa.operand(f"length[{name}]", ln_off + 8 * o, 1, 0, 1, 8, 8)
        oa.expect(f"length[{name}]", np.array([b.length[o]], np.int64))
    oa.device()
    base = oa.region().data_ptr()
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, NOBJ) == 0
    av = tens(b.done)
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, pieces, stride, k, L, m, NOBJ, C.c_void_p(av.data_ptr()),
               m, None, None) == 0
    before = sa.after().copy()
    assert raw(ctx1, "rlnc_decode_stream_deliver", state, nbytes, pieces, stride, k, L, m, NOBJ,
               C.c_void_p(la.region().data_ptr()), C.c_void_p(base), C.c_void_p(base + st_off),
               C.c_void_p(base + ln_off), C.c_void_p(qa.region().data_ptr()), plan_bytes) == 0, ctx1.lib.rlnc_last_error()
    oa.check_device()
    assert np.array_equal(sa.after(), before), "the state changed"
    pa.check_device()
    la.check_device()
    qa.check_guards(qa.after())


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def test_refusals(ctx1):
    import rlnc_amd
    from rlnc_amd import batch as rb

    k, m, L = REFUSAL_SHAPE  # a shape no other test initialises: the library knows a state by its address
    b = batch(k, m, L)
    nbytes = rb.state_bytes(k, m, NOBJ)
    pb = rb.stream_deliver_plan_bytes(k, m, NOBJ)
    buf = dev(np.random.default_rng(60).integers(0, 256, nbytes + 64, dtype=np.uint8))
    plan = dev(np.random.default_rng(61).integers(0, 256, pb + 64, dtype=np.uint8))
    pieces = dev(b.pieces.copy())
    out = Outputs(k, L, seed=62)
    assert buf.data_ptr() % 16 == 0 and plan.data_ptr() % 16 == 0
    state, pp, qp = C.c_void_p(buf.data_ptr()), C.c_void_p(pieces.data_ptr()), C.c_void_p(plan.data_ptr())
    dp, sp, lp = (C.c_void_p(t.data_ptr()) for t in out.args())

    def deliver(ctx=ctx1, st=state, n=nbytes, p=pp, stride=0, k_=k, L_=L, m_=m, nobj=NOBJ, d=dp, s=sp, ln=lp, q=qp, qn=pb):
        return raw(ctx, "rlnc_decode_stream_deliver", st, n, p, stride, k_, L_, m_, nobj, None, d, s, ln, q, qn)

    held = [host(t).copy() for t in (buf, plan, pieces) + out.args()]

    def untouched():
        return all(np.array_equal(host(t), h) for t, h in zip((buf, plan, pieces) + out.args(), held))

    err = ctx1.lib.rlnc_last_error
    assert deliver() == INVALID and b"not initialised" in err() and untouched()  # a state never initialised
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, NOBJ) == 0
    av = tens(b.done)
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, pp, 0, k, L, m, NOBJ, C.c_void_p(av.data_ptr()), m, None,
               None) == 0
    held[0] = host(buf).copy()
    ctx0 = rlnc_amd.Context(0)
    assert deliver(ctx=ctx0) == INVALID and b"rank mode" in err()  # a rank-mode-0 context
    # a state initialised for another shape
    assert deliver(k_=k - 1) == INVALID and deliver(m_=m - 1) == INVALID and deliver(nobj=NOBJ - 1) == INVALID
    assert b"not initialised" in err()
    assert deliver(n=nbytes - 16) == INVALID and deliver(st=C.c_void_p(buf.data_ptr() + 4)) == INVALID
    assert deliver(st=None) == INVALID
    assert deliver(qn=pb - 16) == INVALID and b"plan" in err() and str(pb).encode() in err()  # a short plan buffer
    assert deliver(q=C.c_void_p(plan.data_ptr() + 8)) == INVALID and b"plan" in err()  # a misaligned one
    assert deliver(q=None) == INVALID and b"plan" in err()
    assert deliver(stride=m * (k + L) - 1) == INVALID and b"obj_stride" in err()  # a stride below m(k+L)
    assert deliver(p=None) == INVALID and deliver(d=None) == INVALID and deliver(s=None) == INVALID
    assert deliver(ln=None) == INVALID
    # the crate's checks come first, in push's order; no objects: nothing to do
    assert deliver(k_=0, L_=0, st=None) == 3 and deliver(L_=0, st=None) == 5 and deliver(nobj=0, st=None) == 0
    assert untouched()
    # and the call works
    assert deliver() == 0
    dec, st, ln = out.host()
    for o, name in enumerate(NAMES):
        assert st[o] == b.status[o] and ln[o] == b.length[o], name
        assert np.array_equal(dec[o], b.src[o] if name in FULL else out.fill[0][o]), name
    assert np.array_equal(host(buf), held[0]) and np.array_equal(host(pieces), held[2])


# ---- 7. a receiver that cannot work without the call -----------------------------------------------------------------

def test_a_receiver_delivers_and_retires_on_the_device(ctx1):
    """Six places of (8, 12), L = 4,101.  Arrivals come in seeded rounds, about a third of them useless (a zero vector or a
    combination of what the generation already sent).  A round is push -> deliver -> retire = (status == Ok) -> compact
    with no host read between the four; the checking code reads back afterwards.  A retired place takes the next
    generation, until every place has decoded three; every generation's delivered bytes and length are its source's."""
    import torch

    from oracle import np_oracle as npo
    from rlnc_amd import batch as rb

    k, m, L, nobj, per, want = 8, 12, 4101, 6, 4, 3
    rng = np.random.default_rng(70)
    s = rb.DecodeStream(k, m, nobj, ctx1)
    pieces = torch.zeros((nobj, m, k + L), dtype=torch.uint8, device="cuda:0")
    out = Outputs(k, L, seed=71, nobj=nobj)
    avail, ans = tens([0] * nobj), tens([0] * nobj)

    def generation(o):
        n = k * L - 1 - int(rng.integers(0, k))
        return npo.pad(rng.integers(0, 256, n, dtype=np.uint8), k), n, []

    gen = [generation(o) for o in range(nobj)]
    decoded_count, at, useless = [0] * nobj, [0] * nobj, 0
    last = out.host()
    for rnd in range(60):
        if min(decoded_count) >= want:
            break
        for o in range(nobj):  # the round's arrivals go in from the slot the last compaction answered
            src, _, sent = gen[o]
            rows = []
            for _ in range(per):
                if rng.integers(0, 3) == 0:
                    co = (np_matmul(rng.integers(0, 256, (1, len(sent)), dtype=np.uint8), np.stack(sent))[0]
                          if sent else np.zeros(k, np.uint8))
                    useless += 1
                else:
                    co = rng.integers(1, 256, k, dtype=np.uint8)
                sent.append(co)
                rows.append(co)
            co = np.stack(rows)
            pieces[o, at[o]: at[o] + per] = dev(np.concatenate([co, np_matmul(co, src)], axis=1))
        avail.copy_(tens([a + per for a in at]))
        # ---- the round: no host read from here ...
        s.push(pieces, avail)
        s.deliver(pieces, *out.args())
        retire = (out.status == 0).to(torch.int32)
        s.compact(pieces, retire, None, ans)
        # ---- ... to here
        dec, st, ln = out.host()
        at = host(ans).tolist()
        for o in range(nobj):
            src, n, _ = gen[o]
            if st[o] == 0:
                assert np.array_equal(dec[o], src) and ln[o] == n and at[o] == 0, (rnd, o)
                decoded_count[o] += 1
                gen[o] = generation(o)
            else:
                assert st[o] == NOT_ALL and ln[o] == 0 and np.array_equal(dec[o], last[0][o]) and at[o] < k, (rnd, o)
        last = (dec, st, ln)
    assert min(decoded_count) >= want, decoded_count
    assert useless >= sum(decoded_count) * k // 4  # there was something to reclaim


# ---- 8. capture ------------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch
from oracle import np_oracle as npo
from tests.gpu_util import np_matmul

k, m, L, nobj = 24, 30, 4113, 3  # the 4-wave shared program: its block-table probe must run before the capture
rng = np.random.default_rng(80)
lens = [k * L - 1 - o for o in range(nobj)]
src = np.stack([npo.pad(rng.integers(0, 256, n, dtype=np.uint8), k) for n in lens])
co = rng.integers(1, 256, (nobj, m, k), dtype=np.uint8)
co[:, 2] = 0  # a useless slot: done > rank
p = np.stack([np.concatenate([co[o], np_matmul(co[o], src[o])], axis=1) for o in range(nobj)])
pieces = torch.from_numpy(p).cuda()
ctx = rlnc_amd.Context(0)
ctx.set_rank_mode(1)
cap = batch.DecodeStream(k, m, nobj, ctx)
decoded = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda")
ost = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
dl = torch.full((nobj,), -1, dtype=torch.int64, device="cuda")
avail = torch.zeros(nobj, dtype=torch.int32, device="cuda")
# one eager push and one eager deliver: the plan buffer is allocated and the block table looked up outside the capture
avail.copy_(torch.tensor([3, 0, 1], dtype=torch.int32))
cap.push(pieces, avail, 8)
cap.deliver(pieces, decoded, ost, dl)
torch.cuda.synchronize()
assert ost.cpu().tolist() == [10] * nobj and not decoded.any()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap.push(pieces, avail, 8)
        cap.deliver(pieces, decoded, ost, dl)
rounds = [[5, 9, 1], [12, 9, 20], [20, 26, 20], [30, 26, 24], [30, 26, 30], [30, 30, 30]]
done = [3, 0, 1]
for r in rounds:
    avail.copy_(torch.tensor(r, dtype=torch.int32))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    done = [min(max(a, d), m, d + 8) for d, a in zip(done, r)]
    st = ost.cpu().tolist()
    for o in range(nobj):  # rank k is reached with slot k (slot 2 is useless)
        assert st[o] == (0 if done[o] > k else 10), (r, o, st, done)
        if st[o] == 0:
            assert np.array_equal(decoded[o].cpu().numpy(), src[o]) and int(dl[o]) == lens[o], (r, o)
        else:
            assert not decoded[o].any() and int(dl[o]) == 0, (r, o)
assert ost.cpu().tolist() == [0] * nobj and np.array_equal(decoded.cpu().numpy(), src)
print("stream deliver graph ok")
"""


def test_push_and_deliver_under_graph_capture():
    """One eager push and one eager deliver first, then (push, deliver) captured as one linear graph and replayed over
    the rounds while avail changes: an object is delivered by the replay in which it reaches rank k, and at the end
    every object's decoded bytes are its source."""
    code = CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream deliver graph ok" in r.stdout
