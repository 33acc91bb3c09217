"""GPU: the sender's emit (include/rlnc_hip.h, rlnc_encode_emit; rlnc_amd/csrc/encode_emit.hip;
rlnc_amd.batch.EncodeEmitter) against the numpy model of tests/emit_util.py, which tests/test_encode_emit_host.py holds
to a naive loop.  All comparisons are exact.

An emit must give object o its g_o packets at [base_o, base_o + g_o) in object order -- the random bytes r[i], then
r[i] x src[o] -- write every object id, RLNC_EMIT_NONE from the total on, the count and the grants, and touch no other
byte: every case runs in a footprint arena (tests/footprint.py), so the packets from the total on, the row pads and
the guards must keep their prefill, and src, want and r are compared with their copies."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests import emit_util as eu
from tests.emit_util import emit_model, pattern
from tests.far_address import FAR_ODD, FarArena, FarLayout
from tests.footprint import Arena, assert_inputs_unchanged
from tests.gpu_util import dev, host
from tests.stream_util import raw, true_rank_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 100


def tens(v):
    import torch

    return torch.from_numpy(np.asarray(v, np.int32).reshape(-1).copy()).to("cuda:0")


def up16(v):
    return (v + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def emitter(k, L, nobj, cap, n):
    from rlnc_amd import batch as rb

    return rb.EncodeEmitter(k, L, nobj, cap, n)


def emit_and_check(k, L, cap, want, n, *, out_off=0, pad=0, src_pad=0, seed=0, tag=""):
    """One emit of random sources and random bytes into a prefilled arena holding object, count, granted and the
    packets (`out_off` bytes from a 16-byte boundary, `pad` bytes between packets; `src_pad` bytes between objects of
    src): all four against the model, every other byte of the arena against its prefill, the inputs against their
    copies.  Returns (total, granted)."""
    want = np.asarray(want, np.int32)
    nobj, S = len(want), k + L
    stride = S + pad
    rng = np.random.default_rng(9000 + seed)
    src_buf = rng.integers(0, 256, (nobj, k * L + src_pad), dtype=np.uint8)
    src = src_buf[:, : k * L].reshape(nobj, k, L)
    r = rng.integers(0, 256, (n, k), dtype=np.uint8)
    out, obj, total, g = emit_model(src, want, r, cap)

    c_off = up16(4 * n)
    g_off = c_off + 16
    p_off = up16(g_off + 4 * nobj) + out_off
    ar = Arena(p_off + n * stride, seed=seed + 1, largest_row_stride=stride)
    ar.operand("object", 0, 1, 0, n, 4, 4)
    ar.expect("object", obj)
    ar.operand("count", c_off, 1, 0, 1, 4, 4)
    ar.expect("count", np.array([total], np.int32))
    ar.operand("granted", g_off, 1, 0, nobj, 4, 4)
    ar.expect("granted", g)
    if total:
        ar.operand("out", p_off, 1, 0, total, stride, S)
        ar.expect("out", out)
    ar.device()
    import torch

    reg = ar.region()
    d_obj = reg[: 4 * n].view(torch.int32)
    d_count = reg[c_off: c_off + 4].view(torch.int32)
    d_granted = reg[g_off: g_off + 4 * nobj].view(torch.int32)
    d_out = reg[p_off:].as_strided((n, S), (stride, 1))
    assert d_out.data_ptr() % 16 == out_off % 16
    d_srcbuf, d_want, d_r = dev(src_buf), tens(want), dev(r)
    d_src = d_srcbuf[:, : k * L].view(nobj, k, L)
    emitter(k, L, nobj, cap, n).emit(d_src, d_want, d_r, d_out, d_obj, d_count, d_granted)
    try:
        ar.check_device()
    except AssertionError as e:
        raise AssertionError(f"{tag}: total {total}, granted {g.tolist()[:16]}: {e}") from None
    assert_inputs_unchanged({"src": (src_buf, d_srcbuf), "want": (want, d_want), "r": (r, d_r)})
    return total, g


# ---- 1. the paths ----------------------------------------------------------------------------------------------------

PATHS = [
    # (k, L, cap), want, n, out_off: the path it reaches
    ((1, 4, 1), [1, 0, 1, 1], 5, 0),                      # tail only, one row
    ((3, 4099, 3), [3, 1, 0, 2, 3], 16, 0),               # every grant below 4 across a column block
    ((5, 4096, 4), [4, 1, 4, 2, 3, 4], 20, 0),            # the 1-wave program at four rows, no tail for those objects
    ((16, 4099, 16), [0, 4, 9, 16, 20, -3], 50, 1),       # 2-wave program; clamped wants; out at byte offset 1
    ((24, 8209, 24), [24, 5, 17, 0, 3], 60, 0),           # 4-wave shared program
    ((16, 4100, 70), [70, 65, 64, 33, 6, 0], 240, 0),     # 8-wave program, two row tiles
    ((300, 4099, 8), [8, 3, 5, 0, 7], 30, 0),             # n_in = 300
]


@pytest.mark.parametrize("shape,want,n,out_off", PATHS, ids=[str(p[0]) for p in PATHS])
def test_paths(shape, want, n, out_off):
    k, L, cap = shape
    total, g = emit_and_check(k, L, cap, want, n, out_off=out_off, seed=k + L, tag=shape)
    assert total == int(np.clip(want, 0, cap).sum()) < n and g.tolist() == np.clip(want, 0, cap).tolist()


def test_scan_across_chunks():
    """2,051 objects of (4, 60), at most 2 packets each: zero runs that cover whole chunks of 1,024 objects, the clamps
    in every chunk, one object taking everything, a single packet for the last object."""
    nobj = 2 * eu.CHUNK + 3
    for i, name in enumerate(eu.PATTERNS):
        want = pattern(name, nobj, 2)
        s = int(np.clip(want.astype(np.int64), 0, 2).sum())
        for n in sorted({max(s, 1) + 3, max(s - 1, 1)}):
            total, _ = emit_and_check(4, 60, 2, want, n, seed=10 * i + n % 7, tag=(name, n))
            assert total == min(s, n)


def test_many_objects():
    """65,537 objects of (4, 16), at most one packet each: object ids past 2^16."""
    nobj = 65537
    rng = np.random.default_rng(5)
    want = rng.integers(-1, 3, nobj).astype(np.int32)
    want[-1] = 1
    s = int(np.clip(want, 0, 1).sum())
    total, g = emit_and_check(4, 16, 1, want, s + 3, seed=5, tag="many objects")
    assert total == s > 30000 and g[-1] == 1


# ---- 2. truncation ---------------------------------------------------------------------------------------------------

TRUNC = {
    # w = [0, 4, 9, 16, 16, 0], sum 45: one below the sum; the boundary after object 3; inside the first emitting
    # object; above the sum; object 4 cut from 16 to 2 (from the program to the tail)
    (16, 4099, 16): ([0, 4, 9, 16, 20, -3], [44, 29, 2, 50, 31]),
    # w = [70, 65, 64, 33, 6, 0], sum 238: likewise; 201 cuts object 3 from 33 to 2, 234 object 4 from 6 to 2
    (16, 4100, 70): ([70, 65, 64, 33, 6, 0], [237, 199, 30, 245, 201, 234]),
}


@pytest.mark.parametrize("shape", list(TRUNC), ids=str)
def test_truncation(shape):
    k, L, cap = shape
    want, ns = TRUNC[shape]
    w = np.clip(want, 0, cap)
    moved = 0
    for n in ns:
        total, g = emit_and_check(k, L, cap, want, n, seed=n, tag=(shape, n))
        assert total == min(int(w.sum()), n)
        moved += int(((w >= 4) & (g >= 1) & (g < 4)).sum())
    assert moved >= 2  # an object went from the program to the tail at least twice


# ---- 3. strides ------------------------------------------------------------------------------------------------------

def test_strides():
    """out_stride = k + L + 37 and src_obj_stride = k L + 4,096, together and each alone, out at byte offsets 0 and 5."""
    k, L, cap = 16, 4099, 16
    want = [7, 16, 0, 2, 11]
    for i, (pad, src_pad, off) in enumerate([(37, 4096, 0), (37, 0, 5), (0, 4096, 0)]):
        emit_and_check(k, L, cap, want, 40, out_off=off, pad=pad, src_pad=src_pad, seed=30 + i, tag=(pad, src_pad, off))


def test_far_packets():
    """out_stride = 2^32 + 4,097: packet 1 lies more than 4 GiB from packet 0 (the 64-bit base_o x out_stride)."""
    import torch

    k, L, cap, n = 3, 4099, 2, 2
    S = k + L
    base = 8192 + 16 + 5
    want = np.array([1, 0, 2], np.int32)  # object 2 is cut to one packet
    rng = np.random.default_rng(40)
    src = rng.integers(0, 256, (3, k, L), dtype=np.uint8)
    r = rng.integers(0, 256, (n, k), dtype=np.uint8)
    out, obj, total, g = emit_model(src, want, r, cap)
    assert total == 2 and obj.tolist() == [0, 2] and g.tolist() == [1, 0, 1]
    torch.cuda.empty_cache()
    arena = FarArena(FAR_ODD + (1 << 26))
    try:
        lay = FarLayout(41, arena.size)
        for i in range(total):
            lay.write(f"packet {i}", base + i * FAR_ODD, 1, 0, 1, S, S, out[i])
        lay.build()
        assert len(lay.windows) == 2 and lay.windows[1].lo - lay.windows[0].lo > 1 << 32
        d_out = arena.t.as_strided((n, S), (FAR_ODD, 1), base)
        d_obj, d_count, d_granted = tens([-77] * n), tens([-77]), tens([-77] * 3)
        d_src, d_want, d_r = dev(src), tens(want), dev(r)
        em = emitter(k, L, 3, cap, n)
        arena.run(lay, lambda: em.emit(d_src, d_want, d_r, d_out, d_obj, d_count, d_granted))
        assert host(d_obj).tolist() == obj.tolist() and host(d_count).tolist() == [total]
        assert host(d_granted).tolist() == g.tolist()
        assert_inputs_unchanged({"src": (src, d_src), "want": (want, d_want), "r": (r, d_r)})
    finally:
        arena.t = None
        torch.cuda.empty_cache()


# ---- 4. the loop -----------------------------------------------------------------------------------------------------

def test_loop_with_a_decode_stream():
    """emit -> accept(count = count) -> push -> deliver, want = k - rank + 1 for the unfinished objects computed on the
    device from push's rank, until every object is finished: every round's packets are the model's, and every object's
    delivered bytes are its source with the right length."""
    import torch

    from rlnc_amd import batch as rb

    k, L, nobj = 8, 40, 5
    S, m, cap, n = k + L, 4 * k, k + 1, 40
    rng = np.random.default_rng(50)
    lens = [k * L - 1 - o for o in range(nobj)]  # nobj < k: every object pads to the same L
    src = np.stack([npo.pad(rng.integers(0, 256, ln, dtype=np.uint8), k) for ln in lens])
    assert src.shape == (nobj, k, L)
    d_src = dev(src)
    s = rb.DecodeStream(k, m, nobj, true_rank_context())
    em = rb.EncodeEmitter(k, L, nobj, cap, n)
    pieces = dev(rng.integers(0, 256, (nobj, m, S), dtype=np.uint8))
    out = dev(rng.integers(0, 256, (n, S), dtype=np.uint8))
    objects, count, granted = tens([-7] * n), tens([-7]), tens([-7] * nobj)
    avail, rank = tens([0] * nobj), tens([0] * nobj)
    rounds = 0
    while True:
        want = torch.where(rank < k, k - rank + 1, torch.zeros_like(rank)).to(torch.int32)  # the feedback, on the device
        r = rng.integers(0, 256, (n, k), dtype=np.uint8)
        if rounds == 0:
            r[1: k + 1] = r[0]  # object 0's packets are one vector k + 1 times: it needs a second round
        prev = host(out).copy()
        em.emit(d_src, want, dev(r), out, objects, count, granted)
        s.accept(out, objects, pieces, avail, count=count, finished=True)
        s.push(pieces, avail, None, rank)
        h_want = host(want)
        w_out, w_obj, total, g = emit_model(src, h_want, r, cap)
        assert host(count).tolist() == [total] and np.array_equal(host(objects), w_obj), rounds
        assert np.array_equal(host(granted), g) and np.array_equal(host(out)[:total], w_out), rounds
        assert np.array_equal(host(out)[total:], prev[total:]), rounds
        rounds += 1
        if (host(rank) == k).all():
            break
        assert rounds < 6, host(rank)
    assert rounds >= 2
    dec = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0")
    ost, dl = tens([-7] * nobj), torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0")
    s.deliver(pieces, dec, ost, dl)
    assert host(ost).tolist() == [0] * nobj and host(dl).tolist() == lens
    assert np.array_equal(host(dec), src)


CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch
from tests.emit_util import emit_model

k, L, nobj, cap, n = SHAPE
S, m = k + L, 3 * k
rng = np.random.default_rng(70)
src = rng.integers(0, 256, (nobj, k, L), dtype=np.uint8)


def i32(v):
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device="cuda")


class Side:
    def __init__(self):
        ctx = rlnc_amd.Context(0)
        ctx.set_rank_mode(1)
        self.s = batch.DecodeStream(k, m, nobj, ctx)
        self.em = batch.EncodeEmitter(k, L, nobj, cap, n, ctx)  # a context made before the capture
        self.src = torch.from_numpy(src).cuda()
        self.pieces = torch.from_numpy(fill.copy()).cuda()
        self.out = torch.from_numpy(ofill.copy()).cuda()
        self.r = torch.zeros((n, k), dtype=torch.uint8, device="cuda")
        self.want, self.objects, self.count, self.granted = i32([0] * nobj), i32([-7] * n), i32([-7]), i32([-7] * nobj)
        self.avail, self.rank = i32([0] * nobj), i32([-7] * nobj)

    def write(self, want, r, avail=None):
        self.want.copy_(torch.from_numpy(want))
        self.r.copy_(torch.from_numpy(r))
        if avail is not None:
            self.avail.copy_(torch.tensor(avail, dtype=torch.int32))
        torch.cuda.synchronize()

    def emit(self):
        self.em.emit(self.src, self.want, self.r, self.out, self.objects, self.count, self.granted)

    def call(self):
        self.emit()
        if not EMIT_ONLY:
            self.s.accept(self.out, self.objects, self.pieces, self.avail, count=self.count)
            self.s.push(self.pieces, self.avail, None, self.rank)

    def image(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (self.out, self.objects, self.count, self.granted, self.pieces,
                                                 self.avail, self.rank)]


def inputs(rd):
    want = rng.integers(-2, cap + 3, nobj).astype(np.int32)
    if rd == 1:
        want[:] = cap  # more than n: truncated
    if rd == 2:
        want[:] = 0
    return want, rng.integers(0, 256, (n, k), dtype=np.uint8)


def against_model(side, want, r, before, tag):
    out, objects, count, granted = side.image()[:4]
    w_out, w_obj, total, g = emit_model(src, want, r, cap)
    assert count.tolist() == [total] and np.array_equal(objects, w_obj) and np.array_equal(granted, g), tag
    assert np.array_equal(out[:total], w_out) and np.array_equal(out[total:], before[total:]), tag
    return total


fill = rng.integers(0, 256, (nobj, m, S), dtype=np.uint8)
ofill = rng.integers(0, 256, (n, S), dtype=np.uint8)
cap_side, twin = Side(), Side()
if not EMIT_ONLY:
    first = inputs(0)
    for side in (cap_side, twin):  # one eager round
        side.write(*first)
        side.call()
    assert all(np.array_equal(a, b) for a, b in zip(cap_side.image(), twin.image()))
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        cap_side.call()
emitted = 0
for rd in range(1, 6):
    want, r = inputs(rd)
    avail = [0] * nobj if rd % 2 == 0 else None  # room again now and then
    before = cap_side.image()[0]
    cap_side.write(want, r, avail)
    twin.write(want, r, avail)
    g.replay()
    twin.call()
    emitted += against_model(cap_side, want, r, before, rd)
    for x, y, name in zip(cap_side.image(), twin.image(), ("out", "objects", "count", "granted", "pieces", "avail", "rank")):
        assert np.array_equal(x, y), (rd, name)
assert emitted >= 2 * cap, emitted
print("encode emit graph ok")
"""


def run_child(shape, emit_only):
    code = CHILD.replace("ROOT", repr(ROOT)).replace("SHAPE", repr(shape)).replace("EMIT_ONLY", repr(emit_only))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encode emit graph ok" in r.stdout


def test_loop_under_graph_capture():
    """In a fresh process: one eager round, then (emit, accept, push) captured as one linear graph and replayed five
    times with want and r rewritten in the same tensors: each replay's packets are the model's, and everything equals
    the eager calls on a twin."""
    run_child((16, 100, 4, 20, 40), False)


def test_first_call_inside_a_capture():
    """In a fresh process that has not looked up the 64-row program's block table: the emit's first call is captured
    (the perm product takes every column), and every replay gives the model's bytes -- those of the twin's eager calls,
    which run the program."""
    run_child((16, 4100, 3, 70, 150), True)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------

def test_refusals():
    import rlnc_amd
    from rlnc_amd import batch as rb

    k, L, nobj, cap, n = 6, 50, 4, 5, 12
    S = k + L
    rng = np.random.default_rng(90)
    ctx = rlnc_amd.Context(0)
    pb = rb.encode_emit_plan_bytes(k, cap, nobj, n)
    assert pb > 0 and pb % 16 == 0
    plan = dev(rng.integers(0, 256, pb + 64, dtype=np.uint8))
    src = dev(rng.integers(0, 256, (nobj, k, L), dtype=np.uint8))
    r = dev(rng.integers(0, 256, (n, k), dtype=np.uint8))
    out = dev(rng.integers(0, 256, (n, S), dtype=np.uint8))
    want, objects, count, granted = tens([2, 9, 0, 3]), tens([-77] * n), tens([-77]), tens([-77] * nobj)
    assert plan.data_ptr() % 16 == 0
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def emit(c=ctx, s=ptr(src), sstride=0, k_=k, L_=L, nobj_=nobj, w=ptr(want), cap_=cap, r_=ptr(r), n_=n, o=ptr(out),
             ostride=0, ob=ptr(objects), ct=ptr(count), gr=ptr(granted), q=ptr(plan), qn=pb):
        if c is None:
            return ctx.lib.rlnc_encode_emit(None, s, sstride, k_, L_, nobj_, w, cap_, r_, n_, o, ostride, ob, ct, gr, q, qn)
        return raw(c, "rlnc_encode_emit", s, sstride, k_, L_, nobj_, w, cap_, r_, n_, o, ostride, ob, ct, gr, q, qn)

    every = (plan, src, r, out, want, objects, count, granted)
    held = [host(t).copy() for t in every]

    def untouched():
        return all(np.array_equal(host(t), h) for t, h in zip(every, held))

    err = ctx.lib.rlnc_last_error
    big = 2 ** 50
    # rlnc_encode_batch's order first: the handle, k, L
    assert emit(c=None, k_=0, L_=0) == INVALID
    assert emit(k_=0, L_=0) == 3 and emit(L_=0, n_=0) == 5
    # nothing to do: RLNC_OK before any other check
    assert emit(n_=0, q=None, k_=5000) == 0 and emit(nobj_=0, q=None, o=None) == 0 and emit(cap_=0, q=None, w=None) == 0
    assert untouched()
    # the limits, each by name
    assert emit(k_=eu.MAX_K + 1, qn=big) == INVALID and b"k <= 4096" in err()
    assert emit(cap_=eu.MAX_PER_OBJECT + 1, qn=big) == INVALID and b"max_per_object <= 4096" in err()
    assert emit(n_=eu.MAX_PACKETS + 1, qn=big) == INVALID and b"n <= 1048576" in err()
    assert emit(nobj_=eu.MAX_OBJECTS + 1, qn=big) == INVALID and b"num_objects <= 1048576" in err()
    assert emit(L_=2 ** 40 + 1, qn=big) == INVALID and b"2^40" in err()
    assert emit(ostride=S - 1) == INVALID and b"out_stride" in err()
    assert emit(ostride=2 ** 42 + 1) == INVALID and b"out_stride" in err()
    assert emit(sstride=k * L - 1) == INVALID and b"src_obj_stride" in err()
    # the pointers
    for name in ("s", "w", "r_", "o", "ob", "ct"):
        assert emit(**{name: None}) == INVALID, name
    # the plan: null, misaligned, one byte short, sized for a smaller call
    assert emit(q=None) == INVALID and b"plan" in err()
    assert emit(q=C.c_void_p(plan.data_ptr() + 8), qn=pb) == INVALID and b"plan" in err()
    assert emit(qn=pb - 1) == INVALID and b"plan" in err() and str(pb).encode() in err()
    assert emit(qn=rb.encode_emit_plan_bytes(k, cap, nobj - 1, n)) == INVALID and b"plan" in err()
    assert emit(qn=rb.encode_emit_plan_bytes(k - 1, cap, nobj, n)) == INVALID and b"plan" in err()
    # a launch beyond 2^31 - 1 workgroups (the tail's objects x column blocks); the plan's size does not depend on L
    assert emit(L_=2 ** 36, nobj_=2 ** 10, qn=big) == INVALID and b"workgroups" in err()
    assert untouched()
    # and the call works, on a second context with a plan of its own, without granted
    ctx2 = rlnc_amd.Context(0)
    plan2 = dev(rng.integers(0, 256, pb, dtype=np.uint8))
    w_out, w_obj, total, g = emit_model(held[1], held[4], held[2], cap)
    assert total == 10
    assert emit(c=ctx2, q=ptr(plan2), gr=None) == 0
    assert np.array_equal(host(granted), held[7]) and host(count).tolist() == [total]
    assert np.array_equal(host(objects), w_obj) and np.array_equal(host(out)[:total], w_out)
    assert np.array_equal(host(out)[total:], held[3][total:])
    assert emit() == 0
    assert np.array_equal(host(granted), g) and np.array_equal(host(out)[:total], w_out)
    assert np.array_equal(host(plan)[pb:], held[0][pb:])  # nothing beyond the plan's length
