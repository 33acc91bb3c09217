#!/usr/bin/env python3
"""The two forms of a decode stream's push (rlnc_set_stream_form; include/rlnc_hip.h, "Decode streams") on identical
pieces, at the generation sizes that fit LDS: form 1, the workspace kernels of rank_large.hip (a latch launch, three
launches per block, one more for rank / answered), against form 2, the one-launch LDS kernel of rank_stream.hip.  The
two arms alternate on one context, HIP events around each; WARM warm-ups, then the median and quartiles of TIMED
repetitions.  One JSON line per (row, shape, rounds); `agree` = the two arms' final snapshots (T, statuses, ranks) are
identical -- and, in the single row, identical to the one-shot elimination's.

  single  one push of everything (max_new = m) and the snapshot, per form; beside them one decode_batch_eliminate (the
          one-shot LDS kernel of rank.hip, decode path 0).
  rounds  arrivals in R rounds (round r fills every object's slots up to ceil(m * r / R)), R = 1, 4, 16, 64 and R = m
          (one piece per push): R pushes with max_new = the largest round, rank and answered asked for as a receiver
          does, and one snapshot at the end.  per_push_us = the arm's time over R.

`lds_wins` = form 2's median is below form 1's by more than the two arms' interquartile ranges together: the lines the
automatic rule (RLNC_STREAM_FORM_AUTO) may cover.

    python scripts/decode_stream_lds_timing.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.large_generation_timing import coefficients, quart  # noqa: E402

WARM, TIMED = 3, 25
ROUNDS = (1, 4, 16, 64)
WORKSPACE, LDS = 1, 2
# (objects, k, m); the last two were added to place the automatic rule's edge between k = 32 and k = 64
SHAPES = [(32, 32, 32), (4096, 16, 24), (1024, 16, 24), (64, 64, 72), (64, 128, 136), (1, 200, 210), (64, 200, 210),
          (64, 32, 64), (64, 48, 56)]
DENSITIES = (0, 4)


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

    def arms(rec, ts):
        w, l = quart(ts[WORKSPACE]), quart(ts[LDS])
        spread = (w["ms_q75"] - w["ms_q25"]) + (l["ms_q75"] - l["ms_q25"])
        rec.update({"workspace_ms": w["ms"], "workspace_ms_q25": w["ms_q25"], "workspace_ms_q75": w["ms_q75"],
                    "lds_ms": l["ms"], "lds_ms_q25": l["ms_q25"], "lds_ms_q75": l["ms_q75"],
                    "workspace_over_lds": round(w["ms"] / l["ms"], 3), "lds_wins": bool(w["ms"] - l["ms"] > spread)})
        return rec

    for n, k, m in SHAPES:
        assert batch.stream_lds_fits(k, m)
        for density in DENSITIES:
            co = coefficients(np.random.default_rng(k * 13 + density), n, k, m, density)
            pieces = torch.zeros((n, m, k + 16), dtype=torch.uint8, device="cuda")
            pieces[:, :, :k] = torch.from_numpy(co).cuda()
            full = elim_bufs(n, k, m)
            snaps = {WORKSPACE: elim_bufs(n, k, m), LDS: elim_bufs(n, k, m)}
            rank, answered = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
            everything = torch.full((n,), m, dtype=torch.int32, device="cuda")
            shape = {"shape": f"k{k} m{m} x{n} {'dense' if density == 0 else 'density %d' % density}", "objects": n,
                     "k": k, "m": m, "density": density}

            def timed(avails, most):
                """One repetition per form: a fresh stream (its init is not timed), the pushes, the snapshot."""
                t = {}
                for form in (WORKSPACE, LDS):
                    stream = batch.DecodeStream(k, m, n, ctx)
                    ctx.set_stream_form(form)

                    def pushes():
                        for av in avails:
                            stream.push(pieces, av, most, rank, answered)
                        stream.snapshot(*snaps[form])

                    t[form] = event_ms(pushes)
                ctx.set_stream_form(0)
                return t

            # ---- one push of everything, and the one-shot elimination ------------------------------------------------
            ts = {WORKSPACE: [], LDS: [], "one_shot": []}
            for it in range(WARM + TIMED):
                t = timed([everything], m)
                t["one_shot"] = event_ms(lambda: batch.decode_batch_eliminate(pieces, k, *full, ctx))
                if it >= WARM:
                    for key, v in t.items():
                        ts[key].append(v)
            agree = all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(snaps[WORKSPACE], snaps[LDS], full))
            o = quart(ts["one_shot"])
            emit(arms({"row": "single", **shape, "timed": "push(max_new = m, rank, answered) + snapshot per form | "
                       "decode_batch_eliminate path 0, HIP events", "one_shot_ms": o["ms"],
                       "one_shot_ms_q25": o["ms_q25"], "one_shot_ms_q75": o["ms_q75"],
                       "full_rank": int((full[2] == k).sum()), "agree": agree}, ts))

            # ---- arrivals in R rounds --------------------------------------------------------------------------------
            for R in ROUNDS + (m,):
                upto = [-(-m * r // R) for r in range(1, R + 1)]
                most = max(b - a for a, b in zip([0] + upto, upto))
                avails = [torch.full((n,), u, dtype=torch.int32, device="cuda") for u in upto]
                ts = {WORKSPACE: [], LDS: []}
                for it in range(WARM + TIMED):
                    t = timed(avails, most)
                    if it >= WARM:
                        for key, v in t.items():
                            ts[key].append(v)
                agree = all(torch.equal(x, y) and torch.equal(x, z)
                            for x, y, z in zip(snaps[WORKSPACE], snaps[LDS], full))
                rec = arms({"row": "rounds", **shape, "rounds": R, "max_new": most,
                            "timed": "R pushes (rank, answered) + snapshot per form, HIP events", "agree": agree}, ts)
                rec["workspace_per_push_us"] = round(1000 * rec["workspace_ms"] / R, 2)
                rec["lds_per_push_us"] = round(1000 * rec["lds_ms"] / R, 2)
                emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
