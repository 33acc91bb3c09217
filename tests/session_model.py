"""One model of a whole decode-stream session (include/rlnc_hip.h, "Decode streams"): every call of the receive / relay /
send loop, in any order, on one state.  Numpy only: no GPU.

StreamModel holds what a DecodeStream and its caller hold between calls -- the byte image of pieces [obj][m][k+L], avail,
and per object done, the coding vectors pushed since the last compaction or retire and their decoder -- and has one
method per call, each built from the per-call models the single-call suites use: accept_util.accept_model / place,
stream_util.advance, true_rank.TrueRank (the steps of true_rank_model, one piece at a time), stream_util.compact_model's
rule (the Ok slots, in order), gpu_util.np_matmul, oracle/np_oracle.py's marker rule, recode_util's expected output.
SenderModel wraps emit_util.emit_model and replaces the source of a retired place.

schedule(shape, seed) draws a session: a list of operations with all their host-side inputs, decided with the model and
never with a device, so the same list runs with and without a GPU.  tests/test_stream_session_host.py holds the model to
the library's host decoder and every session to the coverage conditions (CONDITIONS);
tests/test_gpu_stream_session.py runs the sessions on the device and compares everything after every operation."""
import collections
import functools
import hashlib

import numpy as np

from oracle import np_oracle as npo
from tests.accept_util import ABSENT, FINISHED, NO_OBJECT, NO_ROOM, accept_model, place
from tests.deliver_util import BAD_FORMAT, NOT_ALL, payload
from tests.emit_util import emit_model
from tests.gpu_util import MUL, np_matmul
from tests.recode_util import NOT_ENOUGH
from tests.stream_util import PENDING, advance
from tests.true_rank import OK, RECEIVED_ALL, TrueRank

AUTO, WORKSPACE, LDS = 0, 1, 2
NOBJ = 6
SEEDS = (0, 1)
# (k, m, L): the smallest shapes at which the kernels behind the calls differ (deliver_util.SHAPES, stream_util.SHAPES,
# limit_shapes)
#   (5, 9, 20)       LDS form by default, one wave per object, products on the perm tail only
#   (16, 20, 4099)   LDS form by default; 2-wave program plus a 3-byte tail
#   (24, 67, 8209)   workspace form by default with three blocks per push; m no multiple of 4; 4-wave shared program
#   (70, 80, 4100)   both forms by choice; 8-wave program, two row tiles
#   (220, 228, 24)   workspace form by default; scans beyond one pass of 256 threads.  The LDS condition holds here
#                    (160,700 of 163,840 bytes), so both forms are drawn
#   (232, 240, 24)   the same just beyond the LDS condition: the one shape here that the LDS form does not take
SHAPES = [(5, 9, 20), (16, 20, 4099), (24, 67, 8209), (70, 80, 4100), (220, 228, 24), (232, 240, 24)]
LDS_FITS = {(5, 9, 20): True, (16, 20, 4099): True, (24, 67, 8209): True, (70, 80, 4100): True, (220, 228, 24): True,
            (232, 240, 24): False}

# the coverage conditions of a session, by the counter of StreamModel.cover / the session's own that proves each
CONDITIONS = {
    "1 NO_ROOM": "no_room", "1 NO_OBJECT": "no_object", "1 FINISHED": "finished", "1 ABSENT": "absent",
    "2 a push that leaves done < avail": "push_cut",
    "2 a push whose avail < done changes nothing": "push_stale_below",
    "2 a compaction directly after a push that left done < avail": "compact_after_cut",
    "2 a deliver and a recode with a mixed select between a cut push and its compaction": "select_after_cut",
    "3 a slot answered ReceivedAllPieces": "received_all",
    "4 a compaction that moves a piece": "compact_moved",
    "5 a compaction where some object is idle": "compact_idle",
    "6 a compaction that drops accepted-but-unpushed arrivals": "compact_dropped",
    "7 a second compaction that changes nothing": "compact_noop",
    "8 a retire of a finished object": "retire_finished", "8 a retire of an unfinished object": "retire_unfinished",
    "9 a retired place that finishes a second generation": "second_generation",
    "10 a deliver with finished and unfinished objects together": "deliver_mixed",
    "11 a deliver answering InvalidDecodedDataFormat": "deliver_bad_format",
    "12 a recode with rank 0, 0 < rank < k and rank k in one call": "recode_all_ranks",
    "13 a select with a zero": "select_zero",
    "14 consecutive pushes in different forms with a compaction between": "form_switch",
}
LDS_ONLY = ("14 consecutive pushes in different forms with a compaction between",)  # the one exemption, where the
#                                                                                     LDS form does not fit

_memo = collections.OrderedDict()  # the last MEMO_ENTRIES products and emits, by their operands' bytes
MEMO_ENTRIES = 512


def _remember(key, make):
    if key in _memo:
        _memo.move_to_end(key)
    else:
        _memo[key] = make()
        while len(_memo) > MEMO_ENTRIES:
            _memo.popitem(last=False)
    return _memo[key]


def _key(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.digest()


def product(coef, rows):
    """np_matmul, remembered by its operands' bytes: the schedule generator and every run of a session ask for the same
    products."""
    def make():
        out = np_matmul(coef, rows)
        out.setflags(write=False)
        return out

    return _remember(_key(coef, rows), make)


def resolved_form(form, k, m):
    """The kernels a push runs (include/rlnc_hip.h, rlnc_set_stream_form)."""
    return form if form != AUTO else (LDS if k <= 48 and m <= 64 else WORKSPACE)


class StreamModel:
    def __init__(self, k, m, L, nobj, seed):
        self.k, self.m, self.L, self.nobj = k, m, L, nobj
        self.pieces = np.random.default_rng([seed, k, m, L, 0x5E55]).integers(0, 256, (nobj, m, k + L), dtype=np.uint8)
        self.avail = np.zeros(nobj, np.int32)
        self.done = [0] * nobj
        self.dec = [TrueRank(k, m) for _ in range(nobj)]
        self.vec = [[] for _ in range(nobj)]  # the coding vectors pushed since the last compaction or retire
        self.form = AUTO
        self.cover = collections.Counter()
        self._last_form = None       # of the last push that advanced an object
        self._compacted = False      # ... and whether a compaction came after it
        self._last_compact = False   # the last state-changing call was a compaction
        self._cut = False            # the last state-changing call was a push that left some done < avail
        self._cut_selects = set()    # the calls with a mixed select since then
        self._retired_finished = set()

    # ---- what the state holds ----------------------------------------------------------------------------------------
    def rank(self, o):
        return self.dec[o].rank

    def ranks(self):
        return [d.rank for d in self.dec]

    def statuses(self, o):
        return list(self.dec[o].st)

    def useful(self, o):
        return [t for t, s in enumerate(self.dec[o].st) if s == OK]

    def T(self, o):
        """[k][done_o]"""
        return self.dec[o].result()[2]

    def prefix(self, o):
        return np.array(self.vec[o], np.uint8).reshape(-1, self.k)

    # ---- the calls ---------------------------------------------------------------------------------------------------
    def set_form(self, form):
        self.form = form

    def accept(self, arrivals, ids, count=None, finished=False):
        """(slot [n], refused [obj]); the image and avail afterwards."""
        fin = np.array([r == self.k for r in self.ranks()]) if finished else None
        slot, avail, refused = accept_model(ids, self.avail, self.m, self.nobj, count, fin)
        self.pieces = place(self.pieces, arrivals, ids, slot)
        self.avail = avail
        for name, code in (("no_room", NO_ROOM), ("no_object", NO_OBJECT), ("finished", FINISHED), ("absent", ABSENT)):
            self.cover[name] += int((slot == code).sum())
        self._last_compact = self._cut = False
        return slot, refused

    def push(self, max_new=None, avail=None):
        """(rank [obj], answered [obj]).  avail: what the call is given instead of the model's own (a stale array)."""
        av = [int(a) for a in (self.avail if avail is None else avail)]
        before = list(self.done)
        new = advance(before, av, self.m, max_new)
        moved = False
        for o in range(self.nobj):
            if av[o] < before[o]:
                assert new[o] == before[o]
                self.cover["push_stale_below"] += 1
            if new[o] < min(max(av[o], before[o]), self.m):
                self.cover["push_cut"] += 1
            for t in range(before[o], new[o]):
                h = self.pieces[o, t, : self.k].copy()
                was = self.dec[o].rank
                if self.dec[o].push(h) == RECEIVED_ALL:
                    self.cover["received_all"] += 1
                self.vec[o].append(h)
                if was < self.k == self.dec[o].rank and o in self._retired_finished:
                    self.cover["second_generation"] += 1
                moved = True
        self.done = new
        self._cut = any(new[o] < min(max(av[o], before[o]), self.m) for o in range(self.nobj))
        self._cut_selects = set()
        if moved:
            f = resolved_form(self.form, self.k, self.m)
            if self._last_form is not None and f != self._last_form and self._compacted:
                self.cover["form_switch"] += 1
            self._last_form, self._compacted = f, False
            self._last_compact = False
        return self.ranks(), list(new)

    def compact(self, retire=None, into_avail=True):
        """(kept [obj][k], answered [obj]).  The kept pieces move in the image whether the call moves them or the caller
        does by `kept`; into_avail: answered is the caller's avail."""
        k = self.k
        if self._cut:
            self.cover["compact_after_cut"] += 1
            self.cover["select_after_cut"] += self._cut_selects == {"deliver", "recode"}
        self._cut = False
        kept = np.full((self.nobj, k), -1, np.int32)
        answered = np.zeros(self.nobj, np.int32)
        changed = False
        for o in range(self.nobj):
            if retire is not None and retire[o]:
                if self.done[o]:
                    self.cover["retire_finished" if self.rank(o) == k else "retire_unfinished"] += 1
                    changed = True
                else:
                    self.cover["retire_empty"] += 1
                if self.rank(o) == k:
                    self._retired_finished.add(o)
                self.dec[o], self.vec[o], self.done[o] = TrueRank(k, self.m), [], 0
                continue
            u = self.useful(o)  # compact_model's u: the prefix's Ok slots
            r = len(u)
            assert r == self.rank(o)
            kept[o, :r], answered[o] = u, r
            if into_avail and self.avail[o] > self.done[o]:
                self.cover["compact_dropped"] += 1
            if r == self.done[o]:
                self.cover["compact_idle"] += 1
                continue
            changed = True
            if any(t != j for j, t in enumerate(u)):
                self.cover["compact_moved"] += 1
            self.pieces[o, :r] = self.pieces[o][u]
            self.dec[o] = self.dec[o].gathered(u)
            self.vec[o] = [self.vec[o][t] for t in u]
            self.done[o] = r
        if into_avail:
            changed = changed or not np.array_equal(self.avail, answered)
            self.avail = answered.copy()
        if self._last_compact and not changed:
            self.cover["compact_noop"] += 1
        self._last_compact, self._compacted = True, True
        return kept, answered

    def _mixed(self, select, call):
        if self._cut and select is not None and np.any(select) and not np.all(select):
            self._cut_selects.add(call)

    def snapshot(self):
        """(T [obj][k][m], statuses [obj][m] with PENDING, rank [obj])"""
        T = np.zeros((self.nobj, self.k, self.m), np.uint8)
        ps = np.full((self.nobj, self.m), PENDING, np.int32)
        for o in range(self.nobj):
            T[o][:, : self.done[o]] = self.T(o)
            ps[o, : self.done[o]] = self.dec[o].st
        return T, ps, np.array(self.ranks(), np.int32)

    def _decoded(self, o):
        d = self.done[o]
        dec = product(self.T(o), self.pieces[o, :d, self.k:]) if d else np.zeros((self.k, self.L), np.uint8)
        if self.rank(o) < self.k:
            return dec, NOT_ALL, 0
        ok, n = npo.final_data_len(dec.reshape(-1))  # the oracle's marker rule
        return dec, (OK if ok else BAD_FORMAT), (n if ok else 0)

    def apply(self):
        """[(decoded [k][L], status, length)] of every object: the product over every object."""
        return [self._decoded(o) for o in range(self.nobj)]

    def deliver(self, select=None):
        """Per object None (unselected) or (decoded or None for an unfinished object, status, length)."""
        out, full, part = [], 0, 0
        self._mixed(select, "deliver")
        for o in range(self.nobj):
            if select is not None and not select[o]:
                out.append(None)
                self.cover["select_zero"] += 1
                continue
            if self.rank(o) < self.k:
                out.append((None, NOT_ALL, 0))
                part += 1
                continue
            out.append(self._decoded(o))
            full += 1
            self.cover["deliver_bad_format"] += out[-1][1] == BAD_FORMAT
        self.cover["deliver_mixed"] += bool(full and part)
        return out

    def recode(self, r, select=None):
        """Per object None (unselected) or (out [count][k+L] or None at rank 0, status, used): recode_util.expected_of's
        product over the useful pieces."""
        out, seen = [], set()
        self._mixed(select, "recode")
        for o in range(self.nobj):
            if select is not None and not select[o]:
                out.append(None)
                self.cover["select_zero"] += 1
                continue
            rk = self.rank(o)
            seen.add(0 if rk == 0 else 2 if rk == self.k else 1)
            if rk == 0:
                out.append((None, NOT_ENOUGH, 0))
            else:
                out.append((product(r[o][:, :rk], self.pieces[o][self.useful(o)]), OK, rk))
        self.cover["recode_all_ranks"] += seen == {0, 1, 2}
        return out


class SenderModel:
    """The sender of a session: src per place, replaced when the place is retired; emit by emit_util.emit_model.  One
    generation of one place, `bad`, carries a payload with a bad marker."""

    def __init__(self, k, L, nobj, seed, cap, bad):
        self.k, self.L, self.nobj, self.seed, self.cap, self.bad = k, L, nobj, seed, cap, bad
        self.gen = [0] * nobj
        self.src = np.stack([self._payload(o) for o in range(nobj)])

    def _payload(self, o):
        rng = np.random.default_rng([self.seed, o, self.gen[o], 0x5EAD])
        return payload(rng, self.k, self.L, o, "badmarker" if (o, self.gen[o]) == self.bad else "plain")[0]

    def replace(self, o):
        self.gen[o] += 1
        self.src[o] = self._payload(o)

    def emit(self, want, r):
        """(out [total][k+L], objects [n], total, granted [obj])"""
        return _remember(_key(self.src, want, r), lambda: emit_model(self.src, want, r, self.cap))


# ---- the wire --------------------------------------------------------------------------------------------------------
def wire(rng, out, ids, nobj, junk_for, history, k, flood=None):
    """What a lossy network makes of the emitted packets: some dropped, some duplicated, some misaddressed (ids < 0 and
    >= nobj), a zero piece, a duplicate and a multiple of an earlier piece thrown in (coded pieces of the same source
    all: they must be useless, not wrong), everything reordered.  (arrivals [n'][S], ids [n'])."""
    S = out.shape[1]
    pk, pid = [], []
    p = min(0.08, 2.0 / k)  # a couple of packets of a generation meet each fate, whatever its size
    for i in range(len(out)):
        u = rng.random()
        if u < p:
            continue  # dropped
        o = int(ids[i])
        if u < 2 * p:
            o = int(rng.choice([-1, -5, nobj, nobj + 3, -2 ** 31, 2 ** 31 - 1]))  # misaddressed
        pk.append(out[i])
        pid.append(o)
        if u > 1 - p:
            pk.append(out[i])  # duplicated
            pid.append(o)
        if o >= 0 and o < nobj:
            history.setdefault(o, []).append(out[i])
    for o in junk_for:
        pk.append(np.zeros(S, np.uint8))  # a zero vector: 0 x src
        pid.append(o)
        if history.get(o):
            old = history[o][int(rng.integers(len(history[o])))]
            pk.append(old)  # a duplicate of an earlier piece
            pid.append(o)
            pk.append(MUL[int(rng.integers(2, 256))][old])  # a multiple of an earlier piece
            pid.append(o)
    if flood is not None:
        o, copies = flood
        old = history[o][0] if history.get(o) else np.zeros(S, np.uint8)
        pk += [old] * copies  # a stuck retransmission: more copies of one piece than the object has slots
        pid += [o] * copies
    if not pk:
        pk.append(np.zeros(S, np.uint8))
        pid.append(-1)
    order = rng.permutation(len(pk))
    return np.stack(pk)[order], np.array(pid, np.int64)[order]


def padded(rng, arrivals, ids, pad, nobj):
    """The arrivals in a buffer of pad more rows than came: seeded bytes and valid ids there, beyond the count."""
    S = arrivals.shape[1]
    a = np.concatenate([arrivals, rng.integers(0, 256, (pad, S), dtype=np.uint8)])
    i = np.concatenate([ids, rng.integers(0, nobj, pad)])
    return a, i.astype(np.int32)


# ---- the schedule ----------------------------------------------------------------------------------------------------
class Session:
    """The models of one session: the receiver / relay A, the second stream B (m = k + 3) fed by A's recodes, the
    sender.  run(op) applies one operation of a schedule and returns what the call must write."""

    def __init__(self, shape, seed, nobj=NOBJ):
        k, m, L = shape
        self.shape, self.seed, self.nobj = shape, seed, nobj
        self.cap = k + 8
        self.n_emit = nobj * self.cap
        self.A = StreamModel(k, m, L, nobj, seed)
        self.B = StreamModel(k, k + 3, L, nobj, seed + 1000)
        self.sender = SenderModel(k, L, nobj, seed, self.cap, bad=(0, 1))

    def stream(self, op):
        return self.A if op.get("stream", "A") == "A" else self.B

    def run(self, op):
        s, kind = self.stream(op), op["op"]
        if kind == "form":  # of the session's one context: both streams push in it
            self.A.set_form(op["form"])
            return self.B.set_form(op["form"])
        if kind == "emit":
            return self.sender.emit(op["want"], op["r"])
        if kind == "refill":
            for o in op["places"]:
                self.sender.replace(o)
            return self.sender.src
        if kind == "accept":
            return s.accept(op["arrivals"], op["ids"], op["count"], op["finished"])
        if kind == "push":
            return s.push(op["max_new"], op["avail"])
        if kind == "compact":
            return s.compact(op["retire"], op["into_avail"])
        if kind == "snapshot":
            return s.snapshot()
        if kind == "apply":
            return s.apply()
        if kind == "deliver":
            return s.deliver(op["select"])
        if kind == "recode":
            return s.recode(op["r"], op["select"])
        raise AssertionError(kind)

    def coverage(self):
        return collections.Counter(self.A.cover)


def describe(op):
    """An operation for a failure message: its name and its small arguments."""
    small = {}
    for key, v in op.items():
        if key == "op":
            continue
        if isinstance(v, np.ndarray):
            small[key] = v.tolist() if v.size <= 16 else f"<{v.dtype} {v.shape}>"
        else:
            small[key] = v
    return f"{op['op']} {small}"


def _i32(v):
    return np.array([int(x) for x in v], np.int32)


@functools.lru_cache(maxsize=None)
def schedule(shape, seed, rounds=None):
    """The operations of the session (shape, seed), each a dict {"op": name, "stream": "A" | "B", inputs...}.  Drawn
    round by round with the session's own model; deterministic."""
    k, m, L = shape
    fits = LDS_FITS[shape] if shape in LDS_FITS else False
    rng = np.random.default_rng([seed, k, m, L, 0x5C4ED])
    ses = Session(shape, seed)
    A, B, nobj = ses.A, ses.B, ses.nobj
    ops = []
    blk = min(32, m)
    cuts = [None, 0, 1, 3, blk - 1, blk, blk + 1]
    cuts = [cuts[i] for i in rng.permutation(len(cuts))]
    counts = [k + 5, 1, 3, k]
    rounds = rounds or (8 if k < 70 else 6)  # the model's time: about two seconds a session at most
    cut_turn = [0, 0]  # the turns of the cuts and of the form settings
    history = {}
    leave_out, left_out = 2, False
    sel_turn = [0, 0, 0]  # the turns of a read's deliver select, recode select and kind
    pending_b = set()  # places of B to retire: A's place took a new generation

    def next_cut():
        cut_turn[0] += 1
        return cuts[(cut_turn[0] - 1) % len(cuts)]

    def do(op):
        ops.append(op)
        return ses.run(op)

    def form_for(s, want):
        """Some setting that runs the form `want` (None: any setting)."""
        if not fits:
            choices = [AUTO, WORKSPACE]
        elif want is None:
            choices = [AUTO, WORKSPACE, LDS]
        else:
            choices = [f for f in (AUTO, WORKSPACE, LDS) if resolved_form(f, s.k, s.m) == want]
        cut_turn[1] += 1  # the settings take turns
        do({"op": "form", "stream": "A" if s is A else "B", "form": choices[cut_turn[1] % len(choices)]})

    def select_mask(kind):
        if kind == 0:
            return None
        if kind == 1:
            return np.zeros(nobj, np.int32)
        sel = rng.integers(0, 2, nobj).astype(np.int32)
        sel[0], sel[int(rng.integers(1, nobj))] = 1, 0
        return sel

    def reads(s, n):
        """n read-only calls on s, drawn."""
        name = "A" if s is A else "B"
        for _ in range(n):
            what = sel_turn[2] % 4
            sel_turn[2] += 1
            if what == 0:
                do({"op": "snapshot", "stream": name})
            elif what == 1:
                do({"op": "apply", "stream": name})
            elif what == 2:
                sel_turn[0] += 1
                do({"op": "deliver", "stream": name, "select": select_mask(sel_turn[0] % 3)})
            else:
                c = int(rng.choice([1, 3]))
                do({"op": "recode", "stream": name, "r": rng.integers(0, 256, (nobj, c, k), dtype=np.uint8),
                    "select": select_mask(sel_turn[1] % 3)})
                sel_turn[1] += 1

    for t in range(rounds):
        ranks = A.ranks()
        # the sender's feedback: places 0 and 1 at full speed, 2 a third of a generation per round, 3 and 5 a trickle
        # (5 from round 2 on), 4 nothing but what the wire throws in
        want = np.zeros(nobj, np.int32)
        for o in range(nobj):
            need = k - ranks[o]
            if o in (0, 1):
                want[o] = need + 5 if need else 3  # a finished place not yet retired: the sender has not heard
            elif o == 2:
                want[o] = min(need, k // 3 + 1)
            elif o == 3 or (o == 5 and t >= 2):
                want[o] = min(need, 1 + (t + o) % 3)
        if t == 1:
            want[1] = -3  # clamped: nothing
        out, eobj, total, _ = do({"op": "emit", "want": want, "r": rng.integers(0, 256, (ses.n_emit, k), dtype=np.uint8)})
        arr, ids = wire(rng, out[:total], eobj[:total], nobj, [4, 3, int(rng.integers(nobj))], history, k,
                        flood=(next(o for o in (2, 3, 5, 1, 0, 4) if ranks[o] < k), m + 2) if t == 3 else None)
        pad = int(rng.choice([0, 3, 5]))
        arr, ids = padded(rng, arr, ids, pad, nobj)
        n = len(ids)
        count = n - pad if pad else (None if rng.random() < 0.5 else n - 1)
        do({"op": "accept", "stream": "A", "arrivals": arr, "ids": ids, "count": count,
            "finished": bool(t % 4 != 0 or left_out)})
        left_out = False
        kind = t % 4
        if kind == 1:
            # the round whose compaction follows a cut push: the largest of 1, 3 and B - 1 that leaves something unpushed
            room = max(int(A.avail[o]) - A.done[o] for o in range(nobj))
            cut = max([c for c in (1, 3, blk - 1) if c < room], default=1)
        else:
            cut = next_cut()
        first_form = [LDS, WORKSPACE][(t + seed) % 2] if fits else None
        if kind == 2:
            # a compaction with the arrivals accepted and not pushed: they are dropped, their bytes stay
            reads(A, 1)
            do({"op": "compact", "stream": "A", "retire": None, "with_pieces": True, "into_avail": True})
            form_for(A, first_form)
            do({"op": "push", "stream": "A", "max_new": cut, "avail": None})
            do({"op": "push", "stream": "A", "max_new": None, "avail": None})
        else:
            form_for(A, first_form)
            do({"op": "push", "stream": "A", "max_new": cut, "avail": None})
            if kind == 1:
                # a deliver and a recode with a select of zeros and ones while the push is partial
                do({"op": "deliver", "stream": "A", "select": select_mask(2)})
                do({"op": "recode", "stream": "A", "r": rng.integers(0, 256, (nobj, 3, k), dtype=np.uint8),
                    "select": select_mask(2)})
            else:
                reads(A, 1)
            if kind == 1:
                # a compaction after a cut push, the caller's avail left stale above answered: the next push takes the
                # slots again (pieces of the same source, useless now)
                do({"op": "compact", "stream": "A", "retire": None, "with_pieces": bool(t % 8 == 1),
                    "into_avail": False})
                if rng.random() < 0.5:
                    form_for(A, None)
            # a push with a stale avail: below done where something is done, above m where the slots are full
            stale = A.avail.copy()
            for o in range(nobj):
                if A.avail[o] == m:
                    stale[o] = m + 3
                elif A.done[o] and rng.random() < 0.6:
                    stale[o] = int(rng.choice([A.done[o] - 1, 0, -3]))
            do({"op": "push", "stream": "A", "max_new": next_cut(), "avail": stale})
            do({"op": "push", "stream": "A", "max_new": None, "avail": None})
        # stragglers between the pushes and the delivery, when done and rank have parted: an old piece again for every
        # object that has one, the finished ones (refused) included
        late = [o for o in range(nobj) if history.get(o)]
        if late:
            do({"op": "accept", "stream": "A", "ids": np.array(late, np.int32), "count": None, "finished": True,
                "arrivals": np.stack([history[o][int(rng.integers(len(history[o])))] for o in late])})
            do({"op": "push", "stream": "A", "max_new": None, "avail": None})
        reads(A, 2)
        # the round's delivery, the relay's recode into B, and the compaction that retires
        sel = None
        fin = [o for o in range(nobj) if A.rank(o) == k]
        if fin and t >= 1 and leave_out:
            # a finished object is left out: it stays finished into the next round, whose arrivals for it are refused
            sel = np.ones(nobj, np.int32)
            sel[fin[0]] = 0
            leave_out -= 1
            left_out = True
        res = do({"op": "deliver", "stream": "A", "select": sel})
        c = counts[t % len(counts)]
        rsel = None if t % 2 == 0 else select_mask(2)
        r = rng.integers(0, 256, (nobj, c, k), dtype=np.uint8)
        rec = do({"op": "recode", "stream": "A", "r": r, "select": rsel})
        if pending_b:
            do({"op": "compact", "stream": "B", "retire": _i32([o in pending_b for o in range(nobj)]),
                "with_pieces": True, "into_avail": True})
            pending_b.clear()
        # a slot of the staging buffer that recode did not write holds no piece: it is addressed to no object
        rows = np.concatenate([x[0] if x is not None and x[0] is not None else
                               rng.integers(0, 256, (c, k + L), dtype=np.uint8) for x in rec])
        rid = np.repeat([o if x is not None and x[0] is not None else -1 for o, x in enumerate(rec)], c).astype(np.int32)
        do({"op": "accept", "stream": "B", "arrivals": rows, "ids": rid, "count": None, "finished": True})
        form_for(B, None)
        do({"op": "push", "stream": "B", "max_new": None, "avail": None})
        resb = do({"op": "deliver", "stream": "B", "select": None})
        for o, x in enumerate(resb):
            # B's deliveries are the sources: tests/test_stream_session_host.py asserts it of every one
            assert x[0] is None or np.array_equal(x[0], ses.sender.src[o]), (shape, seed, t, o)
        do({"op": "compact", "stream": "B", "retire": _i32([x[0] is not None for x in resb]), "with_pieces": True,
            "into_avail": True})
        retire = np.zeros(nobj, np.int32)
        for o, x in enumerate(res):
            if x is not None and x[0] is not None:
                retire[o] = 1  # delivered, well-formed or not: the place is free
                if x[1] == OK:
                    assert np.array_equal(x[0], ses.sender.src[o]), (shape, seed, t, o)
        if t % 4 == 1:
            retire[3] = 1  # an unfinished object
            retire[5] = 1  # ... and, in round 1, an empty one
        do({"op": "compact", "stream": "A", "retire": retire if (retire.any() or t % 2) else None,
            "with_pieces": bool(t % 3 != 1), "into_avail": True})
        if t % 2 == 0:
            do({"op": "compact", "stream": "A", "retire": None, "with_pieces": bool(t % 4 == 0), "into_avail": True})
        gone = [o for o in range(nobj) if retire[o]]
        if gone:
            do({"op": "refill", "places": gone})
            pending_b.update(gone)
            for o in gone:
                history.pop(o, None)
    for op in ops:
        for v in op.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tuple(ops)


# ---- the whole cycle, round after round (the graph test) -------------------------------------------------------------
GRAPH_SHAPE = (16, 20, 4099)
GRAPH_REPLAYS = 10


class Cycle:
    """The receive / relay / send cycle as one fixed sequence per round -- emit, accept(count, finished), push, deliver,
    recode, retire = (status == Ok), compact(pieces, retire, answered = avail) -- on buffers that live across rounds:
    what tests/test_gpu_stream_session.py captures as one graph.  Between rounds only want (from the rank and the retire
    mask, as the device computes it), the random bytes and the source of the retired places change.  The packet
    capacity is below what the objects ask for, so the first places turn generations over while the later ones starve
    or creep: every round delivers finished, partial and empty objects together."""

    def __init__(self, shape=GRAPH_SHAPE, seed=0, nobj=NOBJ, recode_count=3):
        k, m, L = shape
        self.k, self.m, self.L, self.nobj, self.seed, self.count = k, m, L, nobj, seed, recode_count
        self.cap, self.n = k + 1, 2 * (k + 1) + 3
        self.A = StreamModel(k, m, L, nobj, seed)
        self.sender = SenderModel(k, L, nobj, seed, self.cap, bad=None)
        rng = np.random.default_rng([seed, k, 0xC1C])
        S = k + L
        self.buf = {  # every buffer of the cycle, with its prefill
            "out": rng.integers(0, 256, (self.n, S), dtype=np.uint8),
            "decoded": rng.integers(0, 256, (nobj, k, L), dtype=np.uint8),
            "rout": rng.integers(0, 256, (nobj, recode_count, S), dtype=np.uint8),
            "objects": np.full(self.n, -7, np.int32), "count": np.full(1, -7, np.int32),
            "granted": np.full(nobj, -7, np.int32), "slot": np.full(self.n, -7, np.int32),
            "refused": np.full(nobj, -7, np.int32), "rank": np.zeros(nobj, np.int32),
            "answered": np.full(nobj, -7, np.int32), "ost": np.full(nobj, -7, np.int32),
            "dl": np.full(nobj, -1, np.int64), "rstatus": np.full(nobj, -7, np.int32),
            "rused": np.full(nobj, -7, np.int32), "retire": np.zeros(nobj, np.int32),
            "kept": np.full((nobj, k), -7, np.int32),
        }
        self.refilled = [0] * nobj          # generations a place has taken after a retire
        self.delivered_again = set()        # places that delivered a generation after a refill

    def inputs(self, rd):
        """(want, r [n][k], rr [obj][count][k], the places whose source is replaced first) of round rd."""
        rng = np.random.default_rng([self.seed, rd, 0xC1C])
        b, k = self.buf, self.k
        want = np.where(b["retire"] != 0, k + 1, np.where(b["rank"] < k, k - b["rank"] + 1, 0)).astype(np.int32)
        return (want, rng.integers(0, 256, (self.n, k), dtype=np.uint8),
                rng.integers(0, 256, (self.nobj, self.count, k), dtype=np.uint8), np.flatnonzero(b["retire"]).tolist())

    def step(self, rd):
        """Round rd on the model: every buffer afterwards (buf, plus pieces, avail and src)."""
        b, A = self.buf, self.A
        want, r, rr, gone = self.inputs(rd)
        for o in gone:
            self.sender.replace(o)
            self.refilled[o] += 1
        w_out, obj, total, granted = self.sender.emit(want, r)
        b["out"][:total] = w_out
        b["objects"], b["count"], b["granted"] = obj.astype(np.int32), np.array([total], np.int32), granted
        b["slot"], b["refused"] = A.accept(b["out"], obj, total, True)
        rank, answered = A.push(None)
        b["rank"], b["answered"] = np.array(rank, np.int32), np.array(answered, np.int32)
        for o, (dec, st, n) in enumerate(A.deliver(None)):
            b["ost"][o], b["dl"][o] = st, n
            if dec is not None:
                b["decoded"][o] = dec
                assert st == OK and np.array_equal(dec, self.sender.src[o]), (rd, o)
                if self.refilled[o]:
                    self.delivered_again.add(o)
        for o, (out, st, used) in enumerate(A.recode(rr)):
            b["rstatus"][o], b["rused"][o] = st, used
            if out is not None:
                b["rout"][o] = out
        b["retire"] = (b["ost"] == OK).astype(np.int32)
        b["kept"], _ = A.compact(b["retire"], True)
        return dict(b, pieces=A.pieces, avail=A.avail, src=self.sender.src)
