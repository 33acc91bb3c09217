"""CPU: the session model of tests/session_model.py against the library's host decoder, and every session of
tests/test_gpu_stream_session.py against the coverage conditions, so that the GPU suite cannot pass vacuously.

Model against the host decoder: after every push and every compaction of a session, on either stream, an
rlnc_amd.elimination object in rank mode 1 is fed each changed object's prefix from scratch and must give the model's
rank, statuses and T -- the header's equivalence claim, applied to the model (and to true_rank.TrueRank.gathered, the
model's compaction).  At k <= 24 the same is asked of true_rank_model and stream_util.compact_model.

Coverage: every (shape, seed) session contains each condition of session_model.CONDITIONS at least once, counted by the
model; the shape whose generations do not fit the LDS form is exempt from condition 14 and from nothing else.

The model's own time per session, the drawing of its schedule included (the first, unmemoised run; CPU seconds of one
core of the build machine, seeds 0 / 1): (5, 9, 20) 0.02 / 0.02, (16, 20, 4099) 0.23 / 0.23, (24, 67, 8209) 0.84 / 0.69,
(70, 80, 4100) 1.66 / 1.72, (220, 228, 24) 1.56 / 1.46, (232, 240, 24) 1.64 / 1.66.  The sessions of k >= 70 have six
rounds, the others eight, which keeps them there; every kind of operation is drawn in all of them
(test_a_schedule_is_deterministic_and_draws_every_kind_of_input).  A later run of the same session takes the products
from the module's memo."""
import time

import numpy as np
import pytest

from tests import session_model as sm
from tests.stream_util import compact_model, model_of
from tests.true_rank import host_run

SESSIONS = [(shape, seed) for shape in sm.SHAPES for seed in sm.SEEDS]


def check_decoder(s, o, tag):
    """Object o of stream model s against the host decoder fed its prefix from scratch."""
    vec = s.prefix(o)
    st, rank, T, _ = s.dec[o].result()
    assert len(st) == s.done[o] == len(vec), tag
    if len(vec) == 0:
        assert rank == 0, tag
        return
    h_st, h_rank, h_T, _ = host_run(s.k, vec, fixed=True)
    assert h_st == st and h_rank == rank, (tag, o, h_st, st)
    assert np.array_equal(h_T, T), (tag, o)
    if s.k <= 24:
        m_st, m_rank, m_T, _ = model_of(s.k, vec)
        assert m_st == st and m_rank == rank and np.array_equal(m_T, T), (tag, o)


def run_session(shape, seed, check=True):
    """The session on the model alone: (the Session afterwards, the model's seconds)."""
    ops = sm.schedule(shape, seed)
    ses = sm.Session(shape, seed)
    seen = {}
    spent = 0.0
    ses.relay_delivered = 0
    for i, op in enumerate(ops):
        s = ses.stream(op)
        before = None
        if check and op["op"] == "compact" and s.k <= 24:
            before = [(compact_model(s.k, s.prefix(o)), s.pieces[o].copy()) for o in range(s.nobj)]
        t0 = time.perf_counter()
        res = ses.run(op)
        spent += time.perf_counter() - t0
        if op["op"] == "deliver" and op["stream"] == "B":
            for o, x in enumerate(res):  # the second stream's deliveries are the sources
                if x is not None and x[0] is not None:
                    assert np.array_equal(x[0], ses.sender.src[o]), (shape, seed, i, o)
                    ses.relay_delivered += 1
        if not check or op["op"] not in ("push", "compact"):
            continue
        for o in range(s.nobj):
            key = (op.get("stream", "A"), o)
            now = s.prefix(o).tobytes()
            if seen.get(key) != now:
                seen[key] = now
                check_decoder(s, o, (shape, seed, i, sm.describe(op)))
        if before is not None:
            kept, answered = res
            for o, ((u, r, T, _), img) in enumerate(before):
                if op["retire"] is not None and op["retire"][o]:
                    assert (kept[o] == -1).all() and answered[o] == 0 and np.array_equal(s.pieces[o], img)
                    continue
                assert list(kept[o, :r]) == u and (kept[o, r:] == -1).all() and answered[o] == r
                assert np.array_equal(s.T(o), T)
                assert np.array_equal(s.pieces[o, :r], img[u]) and np.array_equal(s.pieces[o, r:], img[r:])
    return ses, spent


@pytest.mark.parametrize("shape,seed", SESSIONS)
def test_the_session_model_is_the_host_decoder_and_meets_every_condition(shape, seed):
    ses, spent = run_session(shape, seed)
    cover = ses.coverage()
    exempt = () if sm.LDS_FITS[shape] else sm.LDS_ONLY
    missing = [name for name, counter in sm.CONDITIONS.items() if not cover[counter] and name not in exempt]
    print(f"session {shape} seed {seed}: {len(sm.schedule(shape, seed))} operations, model {spent:.2f} s, "
          f"coverage {dict(cover)}")
    assert not missing, (shape, seed, missing)
    assert ses.relay_delivered >= 1, "the second stream delivered nothing"
    kinds = {op["op"] for op in sm.schedule(shape, seed)}
    assert kinds == {"form", "emit", "refill", "accept", "push", "compact", "snapshot", "apply", "deliver", "recode"}


def test_lds_fits_is_what_the_library_says():
    from rlnc_amd import batch

    for (k, m, L), fits in sm.LDS_FITS.items():
        assert batch.stream_lds_fits(k, m) == fits, (k, m)
        assert batch.stream_lds_fits(k, k + 3) == fits, (k, k + 3)  # the second stream of a session


def test_a_schedule_is_deterministic_and_draws_every_kind_of_input():
    shape = sm.SHAPES[0]
    a, b = sm.schedule(shape, 0), sm.schedule.__wrapped__(shape, 0)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            assert np.array_equal(x[key], y[key]) if isinstance(x[key], np.ndarray) else x[key] == y[key], key
    blk = min(32, shape[1])
    for shape_, seed in SESSIONS:
        ops = sm.schedule(shape_, seed)
        blk = min(32, shape_[1])
        pushes = [op for op in ops if op["op"] == "push" and op["stream"] == "A"]
        assert {op["max_new"] for op in pushes} == {None, 0, 1, 3, blk - 1, blk, blk + 1}, (shape_, seed)
        stale = [op["avail"] for op in pushes if op["avail"] is not None]
        assert any((a < 0).any() for a in stale) and any((a > shape_[1]).any() for a in stale), (shape_, seed)
        comp = [op for op in ops if op["op"] == "compact" and op["stream"] == "A"]
        assert {op["with_pieces"] for op in comp} == {True, False} and {op["into_avail"] for op in comp} == {True, False}
        rec = [op for op in ops if op["op"] == "recode"]
        assert {op["r"].shape[1] for op in rec} == {1, 3, shape_[0], shape_[0] + 5}, (shape_, seed)
        for name in ("deliver", "recode"):
            sel = [op["select"] for op in ops if op["op"] == name]
            assert any(s is None for s in sel) and any(s is not None and not s.any() for s in sel), (shape_, seed, name)
        acc = [op for op in ops if op["op"] == "accept" and op["stream"] == "A"]
        assert any(op["count"] is not None and op["count"] < len(op["ids"]) for op in acc)
        assert any((op["ids"] < 0).any() for op in acc) and any((op["ids"] >= sm.NOBJ).any() for op in acc)
        forms = {op["form"] for op in ops if op["op"] == "form"}
        assert forms == ({0, 1, 2} if sm.LDS_FITS[shape_] else {0, 1}), (shape_, seed, forms)


def test_the_graph_cycle_turns_generations_over():
    """The schedule of the graph test, on the model alone: over the eager round and the replays at least two places are
    delivered, retired, refilled and delivered again, and the rounds deliver finished and unfinished objects together,
    recode objects of rank 0, of a partial rank and of rank k in one call."""
    c = sm.Cycle()
    for rd in range(1 + sm.GRAPH_REPLAYS):
        c.step(rd)
    assert len(c.delivered_again) >= 2 and sum(c.refilled) >= 4, (c.delivered_again, c.refilled)
    cover = c.A.cover
    print(f"graph cycle: refilled {c.refilled}, delivered again {sorted(c.delivered_again)}, coverage {dict(cover)}")
    for counter in ("deliver_mixed", "recode_all_ranks", "retire_finished", "second_generation", "compact_idle"):
        assert cover[counter], counter
