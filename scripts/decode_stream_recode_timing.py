#!/usr/bin/env python3
"""A decode stream's recode (rlnc_decode_stream_recode; include/rlnc_hip.h, "Decode streams") against its floor and
against the only route a relay had before it, on identical streams.  The arms alternate on one context; WARM warm-ups,
then the median and quartiles of TIMED repetitions (ROUTE_TIMED for the host route, which is slow at many objects).  One
JSON line per (shape, count, state).

  recode   DecodeStream.recode of every object (select = None): the expand launch, the block-address streams and the
           product over done_o source rows of the objects that hold a useful piece; the others a workgroup that reads
           the state and returns.  HIP events (`recode_ms`) and wall clock between two synchronisations (`recode_wall_ms`).
  floor    (a) rlnc_recode_batch over the same number of useful pieces with n known on the host: the pieces already
           gathered [objects that recode][k][k+L] (the gather is not timed), the same r.  The same product without the
           expand launch and the device-side choice.  HIP events.
  route    (b) what a relay on a stream had to do before: snapshot of the piece statuses, synchronise, read them back,
           pick the Ok slots per object on the host, gather them on the device and rlnc_recode_ragged with one
           descriptor per object.  Wall clock between two synchronisations (it synchronises itself).

States: `compacted` every object at rank k after a compaction (done = k); `uncompacted` every object at rank k with
useless arrivals below done (k/3 of them, capped by m - k, interleaved); `half_rank0` every second object has nothing
pushed, the others are as in `compacted`.  `agree` = after the last repetition the recoded bytes of every recoding
object equal the floor's and the route's, status is Ok / NotEnoughPiecesToRecode and used k / 0.

    python scripts/decode_stream_recode_timing.py profiles/r20_stream_recode.jsonl
    # one line alone, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python ... --shape 0 --count 4 --state compacted)
    python scripts/decode_stream_recode_timing.py --shape 0 --count 4 --state compacted
    python3 scripts/profiles_index.py > profiles/INDEX.md     # the record's entry in the index
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.decode_stream_compact_timing import vectors  # noqa: E402
from scripts.large_generation_timing import quart  # noqa: E402

WARM, TIMED, ROUTE_TIMED = 3, 15, 5
# (objects, k, m, L)
SHAPES = [(64, 32, 40, 1 << 20), (64, 128, 136, 65536), (4096, 16, 24, 4096)]
STATES = ("compacted", "uncompacted", "half_rank0")
OK, NOT_ENOUGH = 0, 6


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--count", type=int, default=None, help="that count alone (default: k and 4)")
    ap.add_argument("--state", default=None, choices=STATES, help="that state alone")
    ap.add_argument("--arm", default=None, choices=("recode", "floor", "route"), help="that arm alone (for a trace)")
    args = ap.parse_args()
    shapes = SHAPES if args.shape is None else [SHAPES[args.shape]]
    states = STATES if args.state is None else (args.state,)
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    ctx = rlnc_amd.Context(0)
    ctx.set_rank_mode(1)
    ctx0 = rlnc_amd.Context(0)  # the floor and the route: the existing recodes

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for n, k, m, L in shapes:
        S = k + L
        bad = min(m - k, k // 3)
        done = k + bad
        co, useful = vectors(np.random.default_rng(k), k, done, bad, "interleaved")
        assert len(useful) == k
        for state in states:
            pieces = torch.randint(0, 256, (n, m, S), dtype=torch.uint8, device="cuda")
            pieces[:, :done, :k] = torch.from_numpy(co).cuda()
            has = np.ones(n, bool)
            if state == "half_rank0":
                has[1::2] = False
            has_d = torch.from_numpy(has).cuda()
            avail = torch.from_numpy(np.where(has, done, 0).astype(np.int32)).cuda()
            stream = batch.DecodeStream(k, m, n, ctx)
            rank = torch.empty((n,), dtype=torch.int32, device="cuda")
            stream.push(pieces, avail, None, rank)
            assert bool((rank == torch.where(has_d, k, 0)).all())
            # the floor's input: the useful pieces of the recoding objects, gathered (not timed)
            gathered = pieces[has_d][:, torch.tensor(useful, device="cuda")].contiguous()
            if state != "uncompacted":
                stream.compact(pieces)
                assert torch.equal(pieces[has_d][:, :k], gathered)
            n_in = done if state == "uncompacted" else k
            ps = torch.empty((n, m), dtype=torch.int32, device="cuda")
            for count in ([k, 4] if args.count is None else [args.count]):
                r = torch.randint(0, 256, (n, count, k), dtype=torch.uint8, device="cuda")
                r_has = r[has_d].contiguous()
                o_rec = torch.zeros((n, count, S), dtype=torch.uint8, device="cuda")
                st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                us = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                o_floor = torch.zeros((int(has.sum()), count, S), dtype=torch.uint8, device="cuda")
                o_route = torch.zeros((n, count, S), dtype=torch.uint8, device="cuda")

                def recode():
                    stream.recode(pieces, r, o_rec, st, us)

                def floor():
                    batch.recode_batch(gathered, r_has, o_floor, k, ctx0)

                def route():
                    stream.snapshot(piece_status=ps)
                    status = ps.cpu().numpy()  # synchronises
                    objs = []
                    for o in range(n):
                        u = np.flatnonzero(status[o] == OK)
                        if len(u) == 0:
                            continue
                        if u[-1] == len(u) - 1:  # a prefix: no gather
                            src = pieces[o, : len(u)]
                        else:
                            src = pieces[o].index_select(0, torch.from_numpy(u).cuda())
                        objs.append((src, r[o, :, : len(u)].contiguous(), o_route[o], k))
                    batch.recode_ragged(objs, ctx0)

                arms = {"recode": recode, "floor": floor, "route": route}
                if args.arm is not None:
                    arms = {args.arm: arms[args.arm]}
                ev = {a: [] for a in arms}
                wl = {a: [] for a in arms}
                for it in range(WARM + TIMED):
                    for a, fn in arms.items():
                        if a == "route":
                            if it < WARM + ROUTE_TIMED:
                                t = wall_ms(fn)
                                if it >= WARM:
                                    wl[a].append(t)
                            continue
                        t = event_ms(fn)
                        w = wall_ms(fn)
                        if it >= WARM:
                            ev[a].append(t)
                            wl[a].append(w)
                rec = {"shape": f"k{k} m{m} x{n} L{L}", "objects": n, "k": k, "m": m, "L": L, "count": count,
                       "state": state, "recoding_objects": int(has.sum()), "n_in": n_in, "useless_below_done": n_in - k,
                       "timed": "arms interleaved; HIP events (ms) and wall clock between synchronisations (wall_ms), "
                                "median of %d (route: wall clock only, %d)" % (TIMED, ROUTE_TIMED)}
                for a in arms:
                    if ev[a]:
                        q = quart(ev[a])
                        rec[a + "_ms"], rec[a + "_ms_q25"], rec[a + "_ms_q75"] = q["ms"], q["ms_q25"], q["ms_q75"]
                    q = quart(wl[a])
                    rec[a + "_wall_ms"], rec[a + "_wall_ms_q25"], rec[a + "_wall_ms_q75"] = q["ms"], q["ms_q25"], q["ms_q75"]
                if args.arm is None:
                    rec["recode_over_floor"] = round(rec["recode_ms"] / rec["floor_ms"], 4)
                    rec["route_over_recode_wall"] = round(rec["route_wall_ms"] / rec["recode_wall_ms"], 4)
                    rec["model_over_floor"] = round(n_in / k, 4)  # a useless slot is a zero column
                    agree = torch.equal(o_rec[has_d], o_floor) and torch.equal(o_route[has_d], o_floor)
                    agree = agree and bool((st == torch.where(has_d, OK, NOT_ENOUGH)).all())
                    agree = agree and bool((us == torch.where(has_d, k, 0)).all()) and not bool(o_rec[~has_d].any())
                    rec["agree"] = bool(agree)
                emit(rec)
                del r, r_has, o_rec, o_floor, o_route
            del stream, pieces, gathered
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
