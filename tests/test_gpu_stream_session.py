"""GPU: whole decode-stream sessions against one model (tests/session_model.py): every call of the receive / relay /
send loop -- emit, accept, push in both forms, compact with retire, snapshot, apply, deliver, recode, a second stream fed
by the first one's recodes -- in the drawn order of session_model.schedule, eager, on one context per session.
tests/test_stream_session_host.py holds the model to the host decoder and every session to the coverage conditions.

After every operation the device is synchronised and everything is compared, exactly: the call's outputs with the
model's (what a call does not write keeps a seeded prefill; deliver's and recode's products lie in a footprint Arena);
the whole pieces buffer of both streams with the model's images; avail; the live state of both streams with that of a
fresh stream of the same shape pushed once with the model's prefix, and the snapshot with the model; the call's inputs
with their copies.  A failure names (shape, seed, operation index), the operation with its arguments, the object and the
first differing byte: run_session(shape, seed, stop=index) reproduces it."""
import ctypes as C

import numpy as np
import pytest

from tests import session_model as sm
from tests.footprint import Arena, assert_inputs_unchanged
from tests.gpu_util import dev, host
from tests.stream_util import check_snapshot, live_state, true_rank_context

pytestmark = pytest.mark.gpu
SESSIONS = [(shape, seed) for shape in sm.SHAPES for seed in sm.SEEDS]


def tens(v):
    import torch

    return torch.tensor([int(x) for x in v], dtype=torch.int32, device="cuda:0")


def same(got, want, what, where):
    """Exact equality of two arrays; the first differing element is named, with the object (the leading index)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (where, what, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        at = tuple(int(x) for x in np.unravel_index(i, want.shape))
        n = int(np.count_nonzero(got != want))
        raise AssertionError(f"{where}: {what} differs first at {at} (object {at[0] if at else 0}): got "
                             f"{got.reshape(-1)[i]}, want {want.reshape(-1)[i]} ({n} elements differ)")


class DeviceStream:
    """A model stream's device side: the stream, its pieces and avail, and a twin that is initialised again and pushed
    the model's prefix whenever the live state is compared."""

    def __init__(self, model, ctx):
        from rlnc_amd import batch

        self.model, self.ctx = model, ctx
        self.s = batch.DecodeStream(model.k, model.m, model.nobj, ctx)
        self.twin = batch.DecodeStream(model.k, model.m, model.nobj, ctx)
        self.pieces = dev(model.pieces)
        self.avail = tens(model.avail)

    def check(self, where):
        import torch

        mo = self.model
        k, m, nobj = mo.k, mo.m, mo.nobj
        same(host(self.pieces), mo.pieces, "pieces [object][slot][byte]", where)
        same(host(self.avail), mo.avail, "avail", where)
        # the twin: a fresh stream of the same shape pushed once with the model's prefix
        t = self.twin
        ctx = self.ctx
        rc = ctx.lib.rlnc_decode_stream_init(ctx.h, C.c_void_p(t.state.data_ptr()), t.state.numel(), k, m, nobj)
        assert rc == 0, (where, rc)
        p2 = np.zeros((nobj, m, k + 1), np.uint8)  # the elimination reads the coefficient bytes alone
        for o in range(nobj):
            p2[o, : mo.done[o], :k] = mo.prefix(o)
        t.push(dev(p2), tens(mo.done))
        torch.cuda.synchronize()
        mine, fresh = live_state(host(self.s.state), k, m, nobj), live_state(host(t.state), k, m, nobj)
        for o in range(nobj):
            assert mine[o][:2] == fresh[o][:2] == (mo.rank(o), mo.done[o]), \
                f"{where}: object {o}: (rank, done) {mine[o][:2]}, a fresh stream's {fresh[o][:2]}, the model's " \
                f"{(mo.rank(o), mo.done[o])}"
            for what, x, y in zip(("piv", "St", "R"), mine[o][2:], fresh[o][2:]):
                same(np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8), f"live state {what} of object {o}", where)
        try:
            check_snapshot(self.s, lambda o, n: mo.dec[o].result(), mo.done, where)
        except AssertionError as e:
            raise AssertionError(f"{where}: snapshot against the model: {e}") from e


def product_arena(res, nobj, rows, width, seed):
    """An Arena over an output [obj][rows][width] in which exactly the objects with a product are the footprint."""
    a = Arena(nobj * rows * width, seed=seed, largest_row_stride=width)
    for o, x in enumerate(res):
        if x is not None and x[0] is not None:
            a.operand(f"object {o}", o * rows * width, 1, rows * width, rows, width, width)
            a.expect(f"object {o}", x[0])
    return a


def run_session(shape, seed, stop=None):
    """The session (shape, seed) on the device and on the model, compared after every operation (up to and including
    operation `stop`)."""
    import torch

    from rlnc_amd import batch

    k, m, L = shape
    S = k + L
    ops = sm.schedule(shape, seed)
    ses = sm.Session(shape, seed)
    nobj = ses.nobj
    assert batch.stream_lds_fits(k, m) == sm.LDS_FITS[shape]
    ctx = true_rank_context()
    side = {"A": DeviceStream(ses.A, ctx), "B": DeviceStream(ses.B, ctx)}
    em = batch.EncodeEmitter(k, L, nobj, ses.cap, ses.n_emit, ctx)
    d_src = dev(ses.sender.src)
    fill = np.random.default_rng([seed, k, 77])
    d_out = dev(fill.integers(0, 256, (ses.n_emit, S), dtype=np.uint8))
    for i, op in enumerate(ops):
        where = f"session {shape} seed {seed} operation {i}: {sm.describe(op)}"
        kind = op["op"]
        d = side[op.get("stream", "A")]
        want = ses.run(op)
        i64 = lambda: torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0")  # noqa: E731
        if kind == "form":
            ctx.set_stream_form(op["form"])
        elif kind == "refill":
            d_src.copy_(dev(want))
        elif kind == "emit":
            w_out, w_obj, total, w_granted = want
            d_want, d_r = tens(op["want"]), dev(op["r"])
            objects, count, granted = tens([-7] * ses.n_emit), tens([-7]), tens([-7] * nobj)
            before = host(d_out).copy()
            em.emit(d_src, d_want, d_r, d_out, objects, count, granted)
            same(host(count), [total], "count", where)
            same(host(objects), w_obj, "objects", where)
            same(host(granted), w_granted, "granted", where)
            same(host(d_out)[:total], w_out, "out [packet][byte]", where)
            same(host(d_out)[total:], before[total:], "out beyond count (prefill)", where)
            assert_inputs_unchanged({"src": (ses.sender.src, d_src), "want": (op["want"], d_want), "r": (op["r"], d_r)})
        elif kind == "accept":
            w_slot, w_refused = want
            d_arr, d_ids = dev(op["arrivals"]), tens(op["ids"])
            d_count = None if op["count"] is None else tens([op["count"]])
            slot, refused = tens([-7] * len(op["ids"])), tens([-7] * nobj)
            d.s.accept(d_arr, d_ids, d.pieces, d.avail, slot, refused, count=d_count, finished=op["finished"])
            same(host(slot), w_slot, "slot", where)
            same(host(refused), w_refused, "refused", where)
            inputs = {"arrivals": (op["arrivals"], d_arr), "ids": (op["ids"], d_ids)}
            if d_count is not None:
                inputs["count"] = (np.array([op["count"]], np.int32), d_count)
            assert_inputs_unchanged(inputs)
        elif kind == "push":
            w_rank, w_done = want
            av = d.avail if op["avail"] is None else tens(op["avail"])
            av_before = host(av).copy()
            rank, answered = tens([-7] * nobj), tens([-7] * nobj)
            d.s.push(d.pieces, av, op["max_new"], rank, answered)
            if op["max_new"] == 0:  # nothing is launched: neither output is written
                w_rank = w_done = [-7] * nobj
            same(host(rank), np.array(w_rank, np.int32), "rank", where)
            same(host(answered), np.array(w_done, np.int32), "answered", where)
            assert_inputs_unchanged({"avail": (av_before, av)})
        elif kind == "compact":
            w_kept, w_answered = want
            retire = None if op["retire"] is None else tens(op["retire"])
            kept = tens([-7] * (nobj * k)).view(nobj, k)
            answered = d.avail if op["into_avail"] else tens([-7] * nobj)
            d.s.compact(d.pieces if op["with_pieces"] else None, retire, kept, answered)
            h_kept = host(kept)
            same(h_kept, w_kept, "kept", where)
            same(host(answered), w_answered, "answered", where)
            if not op["with_pieces"]:
                for o in range(nobj):  # the caller moves its pieces by kept
                    u = [int(x) for x in h_kept[o] if x >= 0]
                    if u:
                        d.pieces[o, : len(u)] = d.pieces[o][u]
            if retire is not None:
                assert_inputs_unchanged({"retire": (op["retire"], retire)})
        elif kind == "snapshot":
            w_T, w_ps, w_rank = want
            T = torch.full((nobj, k, d.model.m), 0xAA, dtype=torch.uint8, device="cuda:0")
            ps, rk = tens([-7] * (nobj * d.model.m)).view(nobj, d.model.m), tens([-7] * nobj)
            d.s.snapshot(T, ps, rk)
            same(host(T), w_T, "T [object][row][slot]", where)
            same(host(ps), w_ps, "piece_status", where)
            same(host(rk), w_rank, "rank", where)
        elif kind == "apply":
            decoded = dev(fill.integers(0, 256, (nobj, k, L), dtype=np.uint8))
            ost, dl = tens([-7] * nobj), i64()
            d.s.apply(d.pieces, decoded, ost, dl)
            same(host(decoded), np.stack([x[0] for x in want]), "decoded [object][row][byte]", where)
            same(host(ost), np.array([x[1] for x in want], np.int32), "object_status", where)
            same(host(dl), np.array([x[2] for x in want], np.int64), "data_len", where)
        elif kind == "deliver":
            sel = None if op["select"] is None else tens(op["select"])
            a = product_arena(want, nobj, k, L, seed=1000 * i + seed)
            a.device()
            ost, dl = tens([-7] * nobj), i64()
            d.s.deliver(d.pieces, a.region().view(nobj, k, L), ost, dl, sel)
            try:
                a.check_device()
            except AssertionError as e:
                raise AssertionError(f"{where}: decoded: {e}") from e
            same(host(ost), np.array([-7 if x is None else x[1] for x in want], np.int32), "object_status", where)
            same(host(dl), np.array([-1 if x is None else x[2] for x in want], np.int64), "data_len", where)
            if sel is not None:
                assert_inputs_unchanged({"select": (op["select"], sel)})
        elif kind == "recode":
            sel = None if op["select"] is None else tens(op["select"])
            count = op["r"].shape[1]
            d_r = dev(op["r"])
            a = product_arena(want, nobj, count, S, seed=1000 * i + seed)
            a.device()
            status, used = tens([-7] * nobj), tens([-7] * nobj)
            d.s.recode(d.pieces, d_r, a.region().view(nobj, count, S), status, used, sel)
            try:
                a.check_device()
            except AssertionError as e:
                raise AssertionError(f"{where}: out: {e}") from e
            same(host(status), np.array([-7 if x is None else x[1] for x in want], np.int32), "status", where)
            same(host(used), np.array([-7 if x is None else x[2] for x in want], np.int32), "used", where)
            inputs = {"r": (op["r"], d_r)}
            if sel is not None:
                inputs["select"] = (op["select"], sel)
            assert_inputs_unchanged(inputs)
        else:
            raise AssertionError(kind)
        for name in ("A", "B"):
            side[name].check(f"{where} [stream {name} afterwards]")
        if stop is not None and i >= stop:
            break
    return ses


@pytest.mark.parametrize("shape,seed", SESSIONS)
def test_a_session_on_the_device_is_the_model_after_every_operation(shape, seed):
    run_session(shape, seed)


# ---- the whole cycle as one graph ------------------------------------------------------------------------------------

CHILD = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
import rlnc_amd
from rlnc_amd import batch
from tests import session_model as sm
from tests.stream_util import live_state

model = sm.Cycle()
k, m, L, nobj, n, count = model.k, model.m, model.L, model.nobj, model.n, model.count
assert L >= 4099
NAMES = ("out", "objects", "count", "granted", "slot", "refused", "pieces", "avail", "rank", "answered", "decoded", "ost",
         "dl", "rout", "rstatus", "rused", "retire", "kept", "src")


class Side:
    def __init__(self):
        ctx = rlnc_amd.Context(0)
        ctx.set_rank_mode(1)
        self.s = batch.DecodeStream(k, m, nobj, ctx)
        self.em = batch.EncodeEmitter(k, L, nobj, model.cap, n, ctx)  # a context made before the capture
        up = lambda a: torch.from_numpy(np.array(a, copy=True)).cuda()
        self.t = {name: up(a) for name, a in model.buf.items()}
        self.t.update(pieces=up(model.A.pieces), avail=up(model.A.avail), src=up(model.sender.src),
                      want=torch.zeros(nobj, dtype=torch.int32, device="cuda"),
                      r=torch.zeros((n, k), dtype=torch.uint8, device="cuda"),
                      rr=torch.zeros((nobj, count, k), dtype=torch.uint8, device="cuda"))

    def write(self, r, rr, gone, src):
        t = self.t
        # want on the device, from the rank the push reported and the retire mask the last round left
        t["want"].copy_(torch.where(t["retire"] != 0, k + 1, torch.where(t["rank"] < k, k - t["rank"] + 1, 0)).to(torch.int32))
        t["r"].copy_(torch.from_numpy(r))
        t["rr"].copy_(torch.from_numpy(rr))
        for o in gone:
            t["src"][o].copy_(torch.from_numpy(src[o]))
        torch.cuda.synchronize()

    def call(self):
        t, s = self.t, self.s
        self.em.emit(t["src"], t["want"], t["r"], t["out"], t["objects"], t["count"], t["granted"])
        s.accept(t["out"], t["objects"], t["pieces"], t["avail"], t["slot"], t["refused"], count=t["count"], finished=True)
        s.push(t["pieces"], t["avail"], None, t["rank"], t["answered"])
        s.deliver(t["pieces"], t["decoded"], t["ost"], t["dl"])
        s.recode(t["pieces"], t["rr"], t["rout"], t["rstatus"], t["rused"])
        t["retire"].copy_((t["ost"] == 0).to(torch.int32))
        s.compact(t["pieces"], t["retire"], t["kept"], t["avail"])

    def image(self):
        torch.cuda.synchronize()
        return {name: self.t[name].cpu().numpy().copy() for name in NAMES}


def check(rd, side, want, twin, tag):
    got = side.image()
    for name in NAMES:
        for other, whose in ((want[name], "the model's"), (twin[name], "the eager twin's")) if twin else ((want[name], "the model's"),):
            if not np.array_equal(got[name], other):
                i = int(np.flatnonzero(got[name].reshape(-1) != np.asarray(other).reshape(-1))[0])
                at = np.unravel_index(i, got[name].shape)
                raise AssertionError(f"round {rd} ({tag}): {name} is not {whose}: first at {tuple(int(x) for x in at)}: "
                                     f"got {got[name].reshape(-1)[i]}, want {np.asarray(other).reshape(-1)[i]}")
    for o, (rank, done, *_rest) in enumerate(live_state(side.s.state.cpu().numpy(), k, m, nobj)):
        assert (rank, done) == (model.A.rank(o), model.A.done[o]), (rd, tag, o, rank, done)
    return got


cap_side, twin = Side(), Side()
steps = []
for rd in range(1 + sm.GRAPH_REPLAYS):
    want_m, r, rr, gone = model.inputs(rd)
    images = model.step(rd)
    for side in (cap_side, twin):
        side.write(r, rr, gone, images["src"])
        assert np.array_equal(side.t["want"].cpu().numpy(), want_m), (rd, "want")
    if rd == 0:  # one eager round: every kernel's first launch and every plan buffer come before the capture
        for side in (cap_side, twin):
            side.call()
        check(rd, cap_side, images, None, "eager")
        check(rd, twin, images, None, "eager twin")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                cap_side.call()
        continue
    g.replay()
    twin.call()
    check(rd, cap_side, images, twin.image(), "replay")
assert len(model.delivered_again) >= 2, model.delivered_again
print("session graph ok", sorted(model.delivered_again), model.refilled)
"""


def test_the_whole_cycle_as_one_graph():
    """(emit, accept(count, finished), push, deliver, recode, retire = (status == Ok), compact(pieces, retire, answered =
    avail)) captured as one linear graph after one eager round, on a shape with L = 4,099, and replayed for ten rounds;
    between replays only want (on the device, from the rank and the retire mask), the random bytes and the source of the
    retired places are rewritten.  After every replay every buffer of the cycle equals the session model's and an eager
    twin's; over the rounds at least two places are delivered, retired, refilled and delivered again
    (tests/test_stream_session_host.py asserts that of the model alone)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD.replace("ROOT", repr(root))], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "session graph ok" in r.stdout
