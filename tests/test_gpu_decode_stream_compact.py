"""GPU: a decode stream's compaction (include/rlnc_hip.h, rlnc_decode_stream_compact; rlnc_amd/csrc/rank_compact.hip;
rlnc_amd.batch.DecodeStream.compact) against the numpy model of tests/stream_util.py;
tests/test_decode_stream_compact_host.py asserts what the batches used here hold.  All comparisons are exact.

After a compaction the live state -- state words 0 and 2, piv[0..rank), St[0..done), R[0..rank)[D] -- must be, byte for
byte, that of a second stream that was initialised and pushed the kept pieces alone; kept / answered must be the
model's; the kept pieces must have moved, all k + L bytes, and nothing else of the pieces buffer or of the state beyond
the documented footprint may change.  The shapes are those of the host file; the piece strides defeat every alignment
and cross a 4,096-byte column chunk of the move (21; 4,099 = one chunk plus 3 bytes; 8,209 = two chunks plus 17)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests.footprint import Arena
from tests.gpu_util import dev, host
from tests.limit_shapes import block_cases, large_layout
from tests.stream_util import (NAMES, SHAPES, cases, check_snapshot, compact_model, i32, kept_models, live_state,
                               model_of, pieces_of, prefix_models, raw, state_words, true_rank_context)
from tests.true_rank import OK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENDING, INVALID = -1, 100
WORKSPACE, LDS = 1, 2
PIECE_CASES = [(5, 7, 21), (16, 20, 4099), (24, 67, 8209)]  # k, m, k + L


@pytest.fixture(scope="module")
def ctx1():
    return true_rank_context()


def tens(v):
    import torch

    return torch.tensor([int(x) for x in v], dtype=torch.int32, device="cuda:0")


def new_stream(ctx, k, m, nobj, pieces, done):
    from rlnc_amd import batch

    s = batch.DecodeStream(k, m, nobj, ctx)
    s.push(pieces, tens(done))
    return s


def want_kept(k, models):
    w = np.full((len(models), k), -1, np.int32)
    for o, (u, r, _, _) in enumerate(models):
        w[o, :r] = u
    return w


def assert_live_equal(a, b, k, m, objects, tag):
    """The live state of stream a equals stream b's for the given objects, byte for byte."""
    nobj = a.num_objects
    la, lb = live_state(host(a.state), k, m, nobj), live_state(host(b.state), k, m, nobj)
    for o in objects:
        assert la[o][:2] == lb[o][:2], (tag, o, la[o][:2], lb[o][:2])
        for what, x, y in zip(("piv", "St", "R"), la[o][2:], lb[o][2:]):
            assert x == y, (tag, o, what)


def fresh_after(ctx, k, m, host_pieces, models):
    """A second stream, initialised and pushed the kept pieces of every object in order."""
    nobj = len(models)
    p2 = np.zeros_like(host_pieces)
    for o, (u, r, _, _) in enumerate(models):
        p2[o, :r] = host_pieces[o][u]
    p2 = dev(p2)
    return new_stream(ctx, k, m, nobj, p2, [r for _, r, _, _ in models]), p2


# ---- 1. equivalence --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", SHAPES)
def test_equivalence(ctx1, k, m):
    """Push a strict prefix, compact: kept / answered are the model's, the live state is a fresh stream's after the kept
    pieces, the snapshot is the model of the kept vectors, and a later push answers as a decoder that saw the kept
    pieces and then the new ones."""
    co, done = cases(k, m)
    nobj, L = co.shape[0], 4
    models = prefix_models(k, m)
    pieces = pieces_of(co, L, seed=k + m)
    before = host(pieces).copy()
    s = new_stream(ctx1, k, m, nobj, pieces, done)
    kept, ans = i32((nobj, k)), i32(nobj)
    s.compact(pieces, None, kept, ans)
    rs = [r for _, r, _, _ in models]
    assert np.array_equal(host(kept), want_kept(k, models))
    assert list(host(ans)) == rs
    ref, _ = fresh_after(ctx1, k, m, before, models)
    assert_live_equal(s, ref, k, m, range(nobj), "compacted")
    after = host(pieces)
    for o, (u, r, _, _) in enumerate(models):
        assert np.array_equal(after[o, :r], before[o][u]) and np.array_equal(after[o, r:], before[o, r:]), NAMES[o]
    check_snapshot(s, lambda o, n: kept_models(k, m)[o], rs, "compacted")
    # new arrivals go into the slots from answered on (at k = 300 three objects, to keep the model short)
    objs = range(nobj) if k <= 24 else [NAMES.index(n) for n in ("mixed", "late", "full")]
    avail, cont = list(rs), {}
    for o in objs:
        n = min(3, m - rs[o])
        new = co[o, done[o]: done[o] + n] if done[o] + n <= m else co[o, :n]
        row = np.random.default_rng(o).integers(0, 256, (len(new), k + L), dtype=np.uint8)
        row[:, :k] = new
        pieces[o, rs[o]: rs[o] + len(new)] = dev(row)
        avail[o] = rs[o] + len(new)
        cont[o] = model_of(k, np.concatenate([co[o][models[o][0]], new]).reshape(-1, k))
    s.push(pieces, tens(avail))
    check_snapshot(s, lambda o, n: cont[o] if o in cont else kept_models(k, m)[o], avail, "continued")


# ---- 2. outliving m --------------------------------------------------------------------------------------------------

def arrivals(rng, k, n):
    """Four objects' coding vectors [4][n][k], each with most arrivals useless and rank k reached near the end (or, for
    the dense one, at once: everything after is ReceivedAllPieces)."""
    from tests.gpu_util import np_matmul

    basis = rng.integers(1, 256, (k, k), dtype=np.uint8)
    slow = np.zeros((n, k), np.uint8)
    for i in range(n):  # a combination of the first 1 + i // 4 basis vectors: at most one new dimension in four
        b = min(k, 1 + i // 4)
        slow[i] = np_matmul(rng.integers(0, 256, (1, b), dtype=np.uint8), basis[:b])[0]
    dense = rng.integers(1, 256, (n, k), dtype=np.uint8)
    junk = rng.integers(1, 256, (n, k), dtype=np.uint8)
    for i in range(n):  # one new piece, then a zero piece, a duplicate and a multiple of it
        if i % 4 == 1:
            junk[i] = 0
        elif i % 4 == 2:
            junk[i] = junk[i - 2]
        elif i % 4 == 3:
            junk[i] = npo.mul_table()[0x53][junk[i - 3]]
    from tests.true_rank import sparse_vectors

    sparse = np.concatenate([sparse_vectors(rng, k, n - k, 2), rng.integers(1, 256, (k, k), dtype=np.uint8)])
    return np.stack([slow, dense, junk, sparse])


def test_a_stream_outlives_its_slots(ctx1):
    """m = k + 4 and 64 >= 3 m arrivals per object, four per round: each round writes the arrivals at answered[o]..,
    pushes and compacts.  After every push the snapshot is the model of (the kept pieces so far + the new arrivals),
    after every compaction the model of the kept pieces; at the end apply returns the source."""
    import torch

    from rlnc_amd import batch

    k, m, L, n, per = 16, 20, 37, 64, 4
    assert n >= 3 * m
    rng = np.random.default_rng(1620)
    co = arrivals(rng, k, n)
    nobj = co.shape[0]
    datas = [rng.integers(0, 256, k * L - 1 - o, dtype=np.uint8) for o in range(nobj)]
    src = np.stack([npo.pad(d, k) for d in datas])
    sent = torch.zeros((nobj, n, k + L), dtype=torch.uint8, device="cuda:0")
    batch.encode_batch(dev(src), dev(co), sent, ctx1)
    pieces = torch.zeros((nobj, m, k + L), dtype=torch.uint8, device="cuda:0")
    s = batch.DecodeStream(k, m, nobj, ctx1)
    held = [[] for _ in range(nobj)]  # the arrival index of the piece in each slot
    kept, ans = i32((nobj, k)), torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
    reclaimed = 0
    for i0 in range(0, n, per):
        at = [int(a) for a in host(ans)]
        assert at == [len(h) for h in held] and max(at) + per <= m
        for o in range(nobj):
            pieces[o, at[o]: at[o] + per] = sent[o, i0: i0 + per]
            held[o] += list(range(i0, i0 + per))
        s.push(pieces, tens([a + per for a in at]))
        models = [model_of(k, co[o][held[o]]) for o in range(nobj)]
        check_snapshot(s, lambda o, _: models[o], [len(h) for h in held], ("pushed", i0))
        s.compact(pieces, None, kept, ans)
        hk = host(kept)
        for o in range(nobj):
            u = [t for t, st in enumerate(models[o][0]) if st == OK]
            assert list(hk[o]) == u + [-1] * (k - len(u)), (i0, o)
            reclaimed += len(held[o]) - len(u)
            held[o] = [held[o][t] for t in u]
        assert list(host(ans)) == [len(h) for h in held]
        models = [model_of(k, co[o][held[o]]) for o in range(nobj)]
        check_snapshot(s, lambda o, _: models[o], [len(h) for h in held], ("compacted", i0))
    assert [len(h) for h in held] == [k] * nobj and reclaimed == nobj * (n - k)
    decoded = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0")
    ost, dl = i32(nobj), torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0")
    s.apply(pieces, decoded, ost, dl)
    assert list(host(ost)) == [OK] * nobj and [int(x) for x in host(dl)] == [d.size for d in datas]
    assert np.array_equal(host(decoded), src)


# ---- 3. pieces -------------------------------------------------------------------------------------------------------

def piece_arena(k, m, S, co, pad=37, base_off=5, seed=300):
    """The pieces of a batch in an arena: piece stride S = k + L, object stride m S + pad, the buffer 5 bytes off a
    16-byte boundary, the headers co and everything else (data, pads, guards) seeded."""
    nobj = co.shape[0]
    stride = m * S + pad
    a = Arena(nobj * stride, seed=seed + S, base_off=base_off, largest_row_stride=S)
    for o in range(nobj):
        for t in range(m):
            at = a.start + o * stride + t * S
            a.fill[at: at + k] = co[o, t]
    a.expected = a.fill.copy()
    t = a.device(seal=False)
    return a, t.as_strided((nobj, m, S), (stride, S, 1), a.start), stride


def expect_moved(a, stride, S, models, skip=()):
    """Slot j of every object not in `skip` holds the old slot u_j, all S bytes; nothing else changes."""
    for o, (u, r, _, _) in enumerate(models):
        if o in skip:
            continue
        base = a.start + o * stride
        for j, uj in enumerate(u):
            a.expected[base + j * S: base + (j + 1) * S] = a.fill[base + uj * S: base + (uj + 1) * S]
            a.mask[base + j * S: base + (j + 1) * S] = uj != j


def check_pieces(ctx, k, m, S):
    co, done = cases(k, m)
    models = prefix_models(k, m)
    a, pieces, stride = piece_arena(k, m, S, co)
    assert pieces.data_ptr() % 16 == 5 and stride > m * S
    s = new_stream(ctx, k, m, co.shape[0], pieces, done)
    a.check_device()  # a push writes no piece byte
    kept, ans = i32((co.shape[0], k)), i32(co.shape[0])
    s.compact(pieces, None, kept, ans)
    expect_moved(a, stride, S, models)
    a.check_device()
    assert np.array_equal(host(kept), want_kept(k, models)) and list(host(ans)) == [r for _, r, _, _ in models]


@pytest.mark.parametrize("k,m,S", PIECE_CASES)
def test_pieces_move_whole_and_nothing_else_changes(ctx1, k, m, S):
    check_pieces(ctx1, k, m, S)


def _aligned_only_main():
    """Child process (RLNC_ASSUME_ALIGNED_ONLY=1): the move on its single-byte path."""
    import rlnc_amd

    c = rlnc_amd.Context(0)
    c.set_rank_mode(1)
    assert c.lib.rlnc_device_unaligned_vector_access(0) == 0
    for case in PIECE_CASES:
        check_pieces(c, *case)
    print("compact aligned-only path ok")


def test_pieces_on_the_aligned_only_path():
    env = dict(os.environ, RLNC_ASSUME_ALIGNED_ONLY="1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--aligned-only"], env=env, capture_output=True,
                       text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "compact aligned-only path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- 4. retire -------------------------------------------------------------------------------------------------------

def test_retire(ctx1):
    """The batch of (24, 67) and the three objects of block_cases; a mask retires five of the twelve.  Those restart
    empty with nothing but their state words written, the others are compacted; a new generation pushed into each
    retired place decodes to its own source."""
    import torch

    from rlnc_amd import batch

    k, m, L, B = 24, 67, 8, 32
    c9, d9 = cases(k, m)
    co = np.concatenate([block_cases(np.random.default_rng(67), k, m, B), c9])
    done = [40, 66, 50] + list(d9)
    nobj = co.shape[0]
    models = [compact_model(k, co[o, :done[o]]) for o in range(nobj)]
    mask = np.zeros(nobj, np.int32)
    mask[[1, 4, 6, 7, 11]] = [1, -1, 7, 1, 2 ** 30]  # any nonzero value; a full, a chain, an idle, an empty, a dense one
    live = [o for o in range(nobj) if not mask[o]]
    assert models[1][1] == k and done[7] == 0 and models[6][1] == done[6]
    pieces = pieces_of(co, L, seed=4)
    before = host(pieces).copy()
    s = new_stream(ctx1, k, m, nobj, pieces, done)
    state0 = state_words(host(s.state), k, m, nobj).copy()
    retire = torch.from_numpy(mask.copy()).to("cuda:0")
    kept, ans = i32((nobj, k)), i32(nobj)
    s.compact(pieces, retire, kept, ans)
    assert np.array_equal(host(retire), mask)
    wk = want_kept(k, models)
    wk[mask != 0] = -1
    assert np.array_equal(host(kept), wk)
    assert list(host(ans)) == [0 if mask[o] else models[o][1] for o in range(nobj)]
    state1 = state_words(host(s.state), k, m, nobj)
    after = host(pieces)
    for o in np.flatnonzero(mask):
        assert list(state1[o][:4]) == [0, 0, 0, 0] and np.array_equal(state1[o][4:], state0[o][4:]), o
        assert np.array_equal(after[o], before[o]), o
    ref, _ = fresh_after(ctx1, k, m, before, [models[o] if not mask[o] else ([], 0, None, []) for o in range(nobj)])
    assert_live_equal(s, ref, k, m, range(nobj), "retired and compacted")  # a retired object: a fresh stream's, empty
    snap = {o: model_of(k, co[o][models[o][0]]) for o in live}
    empty = model_of(k, [])
    rs = [0 if mask[o] else models[o][1] for o in range(nobj)]
    ps, _ = check_snapshot(s, lambda o, n: snap.get(o, empty), rs, "retired")
    assert all((ps[o] == PENDING).all() for o in np.flatnonzero(mask))
    # a new generation into every retired place
    rng = np.random.default_rng(5)
    datas = {o: rng.integers(0, 256, k * L - 3 - o, dtype=np.uint8) for o in np.flatnonzero(mask)}
    src = np.zeros((nobj, k, L), np.uint8)
    co2 = rng.integers(1, 256, (nobj, k + 1, k), dtype=np.uint8)
    co2[:, 2] = co2[:, 1]  # one useless arrival each
    for o, d in datas.items():
        src[o] = npo.pad(d, k)
    sent = torch.zeros((nobj, k + 1, k + L), dtype=torch.uint8, device="cuda:0")
    batch.encode_batch(dev(src), dev(co2), sent, ctx1)
    avail = list(rs)
    for o in datas:
        pieces[o, : k + 1] = sent[o]
        avail[o] = k + 1
    s.push(pieces, tens(avail))
    decoded = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0")
    ost, dl = i32(nobj), torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0")
    s.apply(pieces, decoded, ost, dl)
    for o, d in datas.items():
        assert host(ost)[o] == OK and int(host(dl)[o]) == d.size and np.array_equal(host(decoded)[o], src[o]), o
    check_snapshot(s, lambda o, n: snap[o] if o in snap else model_of(k, co2[o]), avail, "new generation")


# ---- 5. footprint ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_pieces", [True, False])
def test_footprint(ctx1, with_pieces):
    """State and pieces prefilled from a seed.  A compaction writes the four state words, St[0..r), the e part of the
    rows 0..r-1 (all ceil(m/4) dwords), the Q region (scratch) and the moved pieces; piv, the coefficient parts, X, rows
    and statuses from r on, the neighbours, the pads and the guards keep their prefill, and so does every byte of an
    idle object.  Without pieces no piece byte changes."""
    k, m, S = 24, 67, 24 + 13
    co, done = cases(k, m)
    nobj = co.shape[0]
    models = prefix_models(k, m)
    lay = large_layout(k, m)
    kd, me, D = (k + 3) // 4, (m + 3) // 4, lay["D"]
    from rlnc_amd import batch

    nbytes = batch.state_bytes(k, m, nobj)
    sa = Arena(nbytes, seed=520)
    sa.device()
    state = C.c_void_p(sa.region().data_ptr())
    pa, pieces, stride = piece_arena(k, m, S, co, seed=530)
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
    av = tens(done)
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, C.c_void_p(pieces.data_ptr()), stride, k, S - k, m, nobj,
               C.c_void_p(av.data_ptr()), m, None, None) == 0
    before = state_words(sa.after()[sa.start: sa.end], k, m, nobj).copy()
    oa = Arena(nobj * k * 4 + nobj * 4, seed=540)
    oa.operand("kept", 0, nobj, k * 4, k, 4, 4)
    oa.operand("answered", nobj * k * 4, 1, 0, nobj, 4, 4)
    oa.expect("kept", want_kept(k, models))
    oa.expect("answered", np.array([r for _, r, _, _ in models], np.int32))
    oa.device()
    pp = C.c_void_p(pieces.data_ptr()) if with_pieces else None
    assert raw(ctx1, "rlnc_decode_stream_compact", state, nbytes, pp, stride if with_pieces else 0, k,
               S - k if with_pieces else 0, m, nobj, None, C.c_void_p(oa.ptr("kept")),
               C.c_void_p(oa.ptr("answered"))) == 0
    oa.check_device()
    image = sa.after()
    sa.check_guards(image)
    after = state_words(image[sa.start: sa.end], k, m, nobj)
    for o, (u, r, _, st) in enumerate(models):
        may = np.zeros(lay["total"], bool)
        if done[o] > r:
            may[:4] = True
            may[lay["st"]: lay["st"] + r] = True
            may[lay["q"]: lay["q"] + 8 * k] = True
            for i in range(r):
                may[lay["r"] + i * D + kd: lay["r"] + i * D + kd + me] = True
            assert list(after[o][:4]) == [r] * 4 and not after[o][lay["st"]: lay["st"] + r].any(), NAMES[o]
            eb = before[o][lay["r"]: lay["r"] + r * D].reshape(r, D)[:, kd:].copy().view(np.uint8)
            ea = after[o][lay["r"]: lay["r"] + r * D].reshape(r, D)[:, kd:].copy().view(np.uint8)
            assert np.array_equal(ea[:, :r], eb[:, u]) and not ea[:, r:].any(), NAMES[o]
        else:
            assert NAMES[o] in ("idle", "empty")
        stray = np.flatnonzero((after[o] != before[o]) & ~may)
        assert stray.size == 0, (NAMES[o], "dword", int(stray[0]), "of", lay)
    if with_pieces:
        expect_moved(pa, stride, S, models)
    pa.check_device()


# ---- 6. idempotence and forms ----------------------------------------------------------------------------------------

def test_a_second_compaction_writes_nothing_and_the_forms_agree_after_one(ctx1):
    import torch

    from rlnc_amd import batch

    k, m, L = 16, 20, 4
    assert batch.stream_lds_fits(k, m)
    co, done = cases(k, m)
    nobj = co.shape[0]
    models = prefix_models(k, m)
    rs = [r for _, r, _, _ in models]
    pieces = pieces_of(co, L, seed=6)
    s = new_stream(ctx1, k, m, nobj, pieces, done)
    s.compact(pieces)
    state1, pieces1 = host(s.state).copy(), host(pieces).copy()
    kept, ans = i32((nobj, k)), i32(nobj)
    s.compact(pieces, None, kept, ans)
    assert np.array_equal(host(s.state), state1) and np.array_equal(host(pieces), pieces1)
    ident = np.full((nobj, k), -1, np.int32)
    for o, r in enumerate(rs):
        ident[o, :r] = np.arange(r)
    assert np.array_equal(host(kept), ident) and list(host(ans)) == rs
    # two copies of the compacted state (a state is known by its address: each copy is initialised first)
    copies = [batch.DecodeStream(k, m, nobj, ctx1) for _ in range(2)]
    avail, cont = [], []
    for o in range(nobj):
        n = min(3, m - rs[o])
        new = co[o, m - n:]
        row = np.random.default_rng(o).integers(0, 256, (n, k + L), dtype=np.uint8)
        row[:, :k] = new
        pieces[o, rs[o]: rs[o] + n] = dev(row)
        avail.append(rs[o] + n)
        cont.append(model_of(k, np.concatenate([co[o][models[o][0]], new]).reshape(-1, k)))
    try:
        for c, form in zip(copies, (WORKSPACE, LDS)):
            c.state.copy_(s.state)
            ctx1.set_stream_form(form)
            c.push(pieces, tens(avail))
    finally:
        ctx1.set_stream_form(0)
    assert_live_equal(copies[0], copies[1], k, m, range(nobj), "form 1 against form 2")
    for c in copies:
        check_snapshot(c, lambda o, n: cont[o], avail, "after the compaction")


# ---- 7. graph capture ------------------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from oracle import np_oracle as npo
from rlnc_amd import batch
from tests.limit_shapes import block_cases
from tests.true_rank import true_rank_model

k, m, L, n, per = 24, 28, 4, 96, 4
co = block_cases(np.random.default_rng(34), k, n, 32)
nobj = co.shape[0]
rng = np.random.default_rng(1)
datas = [rng.integers(0, 256, k * L - 1 - o, dtype=np.uint8) for o in range(nobj)]
src = np.stack([npo.pad(d, k) for d in datas])
ctx = rlnc_amd.Context(0)
ctx.set_rank_mode(1)
sent = torch.zeros((nobj, n, k + L), dtype=torch.uint8, device="cuda")
batch.encode_batch(torch.from_numpy(src).cuda(), torch.from_numpy(co).cuda(), sent, ctx)
avail = torch.zeros(nobj, dtype=torch.int32, device="cuda")
warm_pieces = torch.zeros((nobj, m, k + L), dtype=torch.uint8, device="cuda")
warm = batch.DecodeStream(k, m, nobj, ctx)  # every kernel's first launch comes before any capture
warm.push(warm_pieces, avail + 2)
warm.compact(warm_pieces)
torch.cuda.synchronize()


def model(vectors):
    return true_rank_model(k, vectors) if len(vectors) else ([], 0, np.zeros((k, 0), np.uint8), None)


def run(order):
    pieces = torch.zeros((nobj, m, k + L), dtype=torch.uint8, device="cuda")
    cap = batch.DecodeStream(k, m, nobj, ctx)
    kept = torch.full((nobj, k), -7, dtype=torch.int32, device="cuda")
    at = torch.zeros(nobj, dtype=torch.int32, device="cuda")
    rank = torch.zeros(nobj, dtype=torch.int32, device="cuda")
    avail.zero_()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            if order == "compact, push":
                cap.compact(None, None, kept, at)
                cap.push(pieces, avail, None, rank)
            else:
                cap.push(pieces, avail, None, rank)
                cap.compact(pieces, None, kept, at)
    T = torch.empty((nobj, k, m), dtype=torch.uint8, device="cuda")
    ps = torch.empty((nobj, m), dtype=torch.int32, device="cuda")
    held = [[] for _ in range(nobj)]  # the arrival in each slot, as the state numbers them

    def keep():
        want = []
        for o in range(nobj):
            u = [t for t, x in enumerate(model(co[o][held[o]])[0]) if x == 0]
            want.append(u + [-1] * (k - len(u)))
            held[o] = [held[o][t] for t in u]
        return want

    for i0 in range(0, n, per):
        if order == "compact, push":
            # the replay compacts what the last push left, then pushes: the next arrivals go where that compaction
            # will answer, which is the rank the last push reported
            nxt = rank.cpu().tolist()
            want_kept = keep()
        else:
            nxt = at.cpu().tolist()
        assert nxt == [len(h) for h in held], (order, i0, nxt)
        for o in range(nobj):
            pieces[o, nxt[o]: nxt[o] + per] = sent[o, i0: i0 + per]
            held[o] += list(range(i0, i0 + per))
        avail.copy_(torch.tensor([x + per for x in nxt], dtype=torch.int32))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if order == "compact, push":
            assert at.cpu().tolist() == nxt, (order, i0, at.cpu().tolist(), nxt)
        else:
            want_kept = keep()
            assert at.cpu().tolist() == [len(h) for h in held], (order, i0)
        assert kept.cpu().tolist() == want_kept, (order, i0)
        T.fill_(0xAA)
        ps.fill_(-7)
        cap.snapshot(T, ps)
        torch.cuda.synchronize()
        for o in range(nobj):
            st, rk, Tm, _ = model(co[o][held[o]])
            d = len(held[o])
            assert ps[o].cpu().tolist() == st + [-1] * (m - d), (order, i0, o)
            assert int(rank[o]) == rk, (order, i0, o)
            assert np.array_equal(T[o].cpu().numpy()[:, :d], Tm) and not T[o].cpu().numpy()[:, d:].any(), (order, i0, o)
    assert rank.cpu().tolist() == [k] * nobj
    return cap, pieces


run("compact, push")
cap, pieces = run("push, compact")
decoded = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda")
ost = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
dl = torch.full((nobj,), -1, dtype=torch.int64, device="cuda")
cap.apply(pieces, decoded, ost, dl)
torch.cuda.synchronize()
assert ost.cpu().tolist() == [0] * nobj and dl.cpu().tolist() == [d.size for d in datas]
assert np.array_equal(decoded.cpu().numpy(), src)
print("stream compact graph ok")
"""


def test_compact_and_push_under_graph_capture():
    """A stream with m = k + 4 sees 96 arrivals per object, four per replay of one captured linear graph; between
    replays the host reads where the next arrivals go, writes them and rewrites avail, and after every replay kept,
    answered and the snapshot are the model's.  Two graphs.  (compact, push): the compaction of what the last push left
    comes first, so the slots it would read may already hold the next arrivals -- it compacts the state alone (no
    pieces) and the receiver keeps its pieces by `kept`, as the header describes.  (push, compact): the pieces move in
    place, the arrivals go in at the compaction's answered, and at the end apply returns the source."""
    code = CHILD.replace("ROOT", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream compact graph ok" in r.stdout


# ---- 8. errors -------------------------------------------------------------------------------------------------------

def test_refusals(ctx1):
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    k, m, nobj, L = 12, 22, 3, 4  # a shape no other test initialises: the library knows a state by its address
    nbytes = batch.state_bytes(k, m, nobj)
    pieces = pieces_of(np.random.default_rng(3).integers(0, 256, (nobj, m, k), dtype=np.uint8), L)
    buf = dev(np.random.default_rng(8).integers(0, 256, nbytes + 64, dtype=np.uint8))
    assert buf.data_ptr() % 16 == 0
    out = i32(nobj * k + nobj)
    state, pp = C.c_void_p(buf.data_ptr()), C.c_void_p(pieces.data_ptr())
    kp, ap = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 4 * nobj * k)

    def compact(st=state, n=nbytes, k_=k, m_=m, nobj_=nobj, ctx=ctx1, L_=L, stride=0, p=pp):
        return raw(ctx, "rlnc_decode_stream_compact", st, n, p, stride, k_, L_, m_, nobj_, None, kp, ap)

    held = [host(buf).copy(), host(pieces).copy(), host(out).copy()]

    def untouched():
        return all(np.array_equal(host(t), h) for t, h in zip((buf, pieces, out), held))

    assert compact() == INVALID and untouched()  # a buffer that was never initialised
    ctx0 = rlnc_amd.Context(0)
    assert raw(ctx1, "rlnc_decode_stream_init", state, nbytes, k, m, nobj) == 0
    av = tens([m - 1] * nobj)
    assert raw(ctx1, "rlnc_decode_stream_push", state, nbytes, pp, 0, k, L, m, nobj, C.c_void_p(av.data_ptr()), m, None,
               None) == 0
    held[0] = host(buf).copy()
    assert compact(ctx=ctx0) == INVALID and b"rank mode" in ctx0.lib.rlnc_last_error()  # a rank-mode-0 context
    assert compact(k_=k - 1) == INVALID and compact(m_=m - 1) == INVALID and compact(nobj_=nobj - 1) == INVALID
    assert compact(stride=m * (k + L) - 1) == INVALID  # a short stride
    assert compact(n=nbytes - 16) == INVALID and compact(st=C.c_void_p(buf.data_ptr() + 4)) == INVALID
    assert compact(st=None) == INVALID
    # the crate's checks, in push's order, and the call that has nothing to do
    assert compact(k_=0, L_=0) == 3 and compact(L_=0) == 5 and compact(nobj_=0) == 0
    assert untouched()
    # without pieces L and the stride are ignored; and the stream works
    assert compact(p=None, L_=0, stride=1) == 0
    torch.cuda.synchronize()
    assert not untouched() and np.array_equal(host(pieces), held[1])
    assert np.array_equal(host(buf)[nbytes:], held[0][nbytes:])


if __name__ == "__main__" and "--aligned-only" in sys.argv:
    _aligned_only_main()
