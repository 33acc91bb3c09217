#!/usr/bin/env python3
"""Decode streams (rlnc_amd.batch.DecodeStream; include/rlnc_hip.h, "Decode streams") against what the library offered
a progressive receiver before them, on identical pieces: the shapes of profiles/r09_large_generation.jsonl, arrivals in
R rounds (round r fills every object's slots up to ceil(m * r / R)).  HIP events around each arm, the two arms
alternating on one context; WARM warm-ups, then the median and quartiles of the timed repetitions (fewer where one
repetition of the re-run arm is long).  One JSON line per (row, shape, R); `agree` = the stream's final snapshot is the
one-shot elimination's T, statuses and ranks.

  rounds  stream: R pushes (max_new = the largest round, so a push is ceil(that / B) blocks) and one snapshot at the
          end.  rerun: decode_batch_eliminate under decode path 7 over each round's prefix, from scratch -- what a
          receiver that wants the rank after every round had to do; about R / 2 times the work of one elimination.
  single  one push of everything (max_new = m) and the snapshot, against one decode_batch_eliminate under path 7: the
          price of the stream form itself (the latch launch, the block read from the state, the statuses of a block met
          at rank k).  For the two shapes that fit LDS, path 7 is the LDS kernel (rank.hip), which a stream does not use.

What came out (one MI355X, profiles/r12_decode_stream.jsonl; beyond LDS, m = k + 8).  single: 1.003-1.010x the one-shot
call, 1-3 us per block, mostly the state reads at the head of reduce and step.  rounds: the stream costs 1.02-1.13x /
1.05-1.24x / 1.03-2.9x one elimination at R = 4 / 16 / 64 and the re-run 1.8-2.6x / 5.2-9.2x / 13.7-19.3x the stream;
the 2.9x is 64 x k = 256 at R = 64, five pieces per push, where every push is a whole block's launches.  Where rank.hip
fits, the stream is what path 8 is: faster for one object of k = 200 (1.34 against 3.86 ms), 1.76x slower at the
bench's 32 x k = 32.

    python scripts/decode_stream_timing.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.large_generation_timing import HOST, RANK_LDS, coefficients, quart  # noqa: E402

WARM, TIMED = 3, 25
ROUNDS = (4, 16, 64)
SHAPES = HOST + RANK_LDS  # (name, objects, k, m, density)


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    ctx = rlnc_amd.Context(0)
    ctx.set_rank_mode(1)
    ctx.set_decode_path(7)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def elim_bufs(n, k, m):
        return (torch.empty((n, k, m), dtype=torch.uint8, device="cuda"),
                torch.empty((n, m), dtype=torch.int32, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"))

    for name, n, k, m, density in SHAPES:
        co = coefficients(np.random.default_rng(k * 13 + density), n, k, m, density)
        pieces = torch.zeros((n, m, k + 16), dtype=torch.uint8, device="cuda")
        pieces[:, :, :k] = torch.from_numpy(co).cuda()
        full = elim_bufs(n, k, m)
        snap = elim_bufs(n, k, m)
        everything = torch.full((n,), m, dtype=torch.int32, device="cuda")
        shape = {"shape": name, "objects": n, "k": k, "m": m, "density": density}

        # ---- one push of everything against one elimination ----------------------------------------------------------
        ts = {"stream": [], "one_shot": []}
        for it in range(WARM + TIMED):
            stream = batch.DecodeStream(k, m, n, ctx)  # its init is not timed

            def single():
                stream.push(pieces, everything, m)
                stream.snapshot(*snap)

            a = event_ms(single)
            b = event_ms(lambda: batch.decode_batch_eliminate(pieces, k, *full, ctx))
            if it >= WARM:
                ts["stream"].append(a)
                ts["one_shot"].append(b)
        agree = all(torch.equal(x, y) for x, y in zip(snap, full))
        s, o = quart(ts["stream"]), quart(ts["one_shot"])
        emit({"row": "single", **shape, "timed": "push(max_new = m) + snapshot | decode_batch_eliminate path 7, HIP "
              "events", "stream_ms": s["ms"], "stream_ms_q25": s["ms_q25"], "stream_ms_q75": s["ms_q75"],
              "one_shot_ms": o["ms"], "one_shot_ms_q25": o["ms_q25"], "one_shot_ms_q75": o["ms_q75"],
              "stream_over_one_shot": round(s["ms"] / o["ms"], 3), "full_rank": int((full[2] == k).sum()),
              "agree": agree})
        one_shot_ms = o["ms"]

        # ---- arrivals in R rounds ------------------------------------------------------------------------------------
        for R in ROUNDS:
            upto = [-(-m * r // R) for r in range(1, R + 1)]
            most = max(b - a for a, b in zip([0] + upto, upto))
            avails = [torch.full((n,), u, dtype=torch.int32, device="cuda") for u in upto]
            prefix = [elim_bufs(n, k, u) for u in sorted(set(upto))]
            prefix = dict(zip(sorted(set(upto)), prefix))
            timed = TIMED if one_shot_ms * R / 2 < 40 else 5  # a repetition of the re-run arm is about R / 2 one-shots
            ts = {"stream": [], "rerun": []}
            for it in range(WARM + timed):
                stream = batch.DecodeStream(k, m, n, ctx)

                def pushes():
                    for av in avails:
                        stream.push(pieces, av, most)
                    stream.snapshot(*snap)

                def rerun():
                    for u in upto:
                        batch.decode_batch_eliminate(pieces[:, :u], k, *prefix[u], ctx)

                a = event_ms(pushes)
                b = event_ms(rerun)
                if it >= WARM:
                    ts["stream"].append(a)
                    ts["rerun"].append(b)
            agree = all(torch.equal(x, y) for x, y in zip(snap, full)) and \
                all(torch.equal(x, y) for x, y in zip(prefix[m], full))
            s, o = quart(ts["stream"]), quart(ts["rerun"])
            emit({"row": "rounds", **shape, "rounds": R, "max_new": most, "repetitions": timed,
                  "timed": "R pushes + snapshot | R decode_batch_eliminate (path 7) over the prefixes, HIP events",
                  "stream_ms": s["ms"], "stream_ms_q25": s["ms_q25"], "stream_ms_q75": s["ms_q75"],
                  "rerun_ms": o["ms"], "rerun_ms_q25": o["ms_q25"], "rerun_ms_q75": o["ms_q75"],
                  "rerun_over_stream": round(o["ms"] / s["ms"], 2),
                  "stream_over_one_shot": round(s["ms"] / one_shot_ms, 3), "agree": agree})
    ctx.set_decode_path(0)
    if out:
        out.close()


if __name__ == "__main__":
    main()
