#!/usr/bin/env python3
"""A decode stream's delivery (rlnc_decode_stream_deliver; include/rlnc_hip.h, "Decode streams") against the way out a
stream had before it, on identical streams.  The arms alternate on one context, HIP events around each; WARM warm-ups,
then the median and quartiles of TIMED repetitions.  Before every arm the pieces and the state are restored (not timed)
to what one push left.  One JSON line per (shape, finished share).

  deliver          DecodeStream.deliver of every object (select = None): the finished ones get their product over
                   done_o source rows, the others a workgroup that reads the state and returns.
  compact_deliver  the same call after a compaction (the compaction is not timed: `compact_ms` is its own median): the
                   finished objects' product over k source rows, the minimum.
  apply            DecodeStream.apply, unchanged: a snapshot of every object's T and rlnc_decode_batch_apply, the dense
                   k x m x L product and the marker scan over every object.

`finished` of the objects hold k useful pieces and as many useless ones as a quarter of the pushed slots asks for and
m - k leaves room for (k/3, capped by m - k); the others hold k/2 useful pieces and a quarter useless.  `model` = the
finished share x done / m, the share of apply's product a delivery should cost before its floor of launches and
returning workgroups.  `agree` = after the last repetition the delivered bytes of every finished object (both delivery
arms) and every object's status and length equal apply's.

    python scripts/decode_stream_deliver_timing.py profiles/r18_stream_deliver.jsonl
    # one line alone, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python ... --shape 0 --finished 1/1)
    python scripts/decode_stream_deliver_timing.py --shape 0 --finished 1/1
    python3 scripts/profiles_index.py > profiles/INDEX.md     # the record's entry in the index
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.decode_stream_compact_timing import vectors  # noqa: E402
from scripts.large_generation_timing import quart  # noqa: E402

WARM, TIMED = 3, 25
# (objects, k, m, L)
SHAPES = [(4096, 16, 24, 4096), (64, 32, 40, 1 << 20), (64, 128, 136, 65536)]
FINISHED = ((1, 64), (1, 8), (1, 2), (1, 1))


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--finished", default=None, help="N/D: that finished share alone")
    args = ap.parse_args()
    shapes = SHAPES if args.shape is None else [SHAPES[args.shape]]
    shares = FINISHED if args.finished is None else (tuple(int(x) for x in args.finished.split("/")),)
    out = open(args.out, "w") if args.out else None

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

    def outputs(n, k, L):
        return (torch.zeros((n, k, L), dtype=torch.uint8, device="cuda"),
                torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                torch.full((n,), -7, dtype=torch.int64, device="cuda"))

    for n, k, m, L in shapes:
        S = k + L
        orig = torch.randint(0, 256, (n, m, S), dtype=torch.uint8, device="cuda")
        pieces = torch.empty_like(orig)
        bad_f = min(m - k, k // 3)
        done_f = k + bad_f
        good_u = k // 2
        bad_u = good_u // 3
        done_u = good_u + bad_u
        co_f, _ = vectors(np.random.default_rng(k), k, done_f, bad_f, "interleaved")
        co_u, _ = vectors(np.random.default_rng(k + 1), k, done_u, bad_u, "interleaved")
        outs = {a: outputs(n, k, L) for a in ("deliver", "compact_deliver", "apply")}
        for num, den in shares:
            nf = max(1, n * num // den)
            fin = np.zeros(n, bool)
            fin[(np.arange(nf) * n) // nf] = True  # spread evenly over the batch
            fin_d = torch.from_numpy(fin).cuda()
            orig[fin_d, :done_f, :k] = torch.from_numpy(co_f).cuda()
            orig[~fin_d, :done_u, :k] = torch.from_numpy(co_u).cuda()
            avail = torch.from_numpy(np.where(fin, done_f, done_u).astype(np.int32)).cuda()
            stream = batch.DecodeStream(k, m, n, ctx)
            rank = torch.empty((n,), dtype=torch.int32, device="cuda")
            stream.push(orig, avail, None, rank)
            assert bool((rank == torch.where(fin_d, k, good_u)).all())
            state0 = stream.state.clone()

            def restore():
                pieces.copy_(orig)
                stream.state.copy_(state0)

            def compacted():
                restore()
                stream.compact(pieces)

            arms = {
                "deliver": (restore, lambda: stream.deliver(pieces, *outs["deliver"])),
                "compact_deliver": (compacted, lambda: stream.deliver(pieces, *outs["compact_deliver"])),
                "apply": (restore, lambda: stream.apply(pieces, *outs["apply"])),
                "compact": (restore, lambda: stream.compact(pieces)),
            }
            ts = {a: [] for a in arms}
            for it in range(WARM + TIMED):
                for a, (prep, fn) in arms.items():
                    prep()
                    t = event_ms(fn)
                    if it >= WARM:
                        ts[a].append(t)
            ref = outs["apply"]
            agree = all(torch.equal(outs[a][0][fin_d], ref[0][fin_d]) and torch.equal(outs[a][1], ref[1]) and
                        torch.equal(outs[a][2], ref[2]) for a in ("deliver", "compact_deliver"))
            agree = agree and bool((ref[1][~fin_d] == 10).all()) and bool((ref[1][fin_d] != 10).all())
            q = {a: quart(v) for a, v in ts.items()}
            rec = {"shape": f"k{k} m{m} x{n} L{L}", "objects": n, "k": k, "m": m, "L": L,
                   "finished": f"{num}/{den}", "finished_objects": int(nf), "done_finished": done_f,
                   "useless_finished": bad_f, "done_unfinished": done_u, "useless_unfinished": bad_u,
                   "timed": "one call per arm on restored pieces and state, HIP events, median of %d" % TIMED}
            for a in arms:
                rec[a + "_ms"], rec[a + "_ms_q25"], rec[a + "_ms_q75"] = q[a]["ms"], q[a]["ms_q25"], q[a]["ms_q75"]
            rec["model"] = round(nf / n * done_f / m, 4)
            rec["deliver_over_apply"] = round(q["deliver"]["ms"] / q["apply"]["ms"], 4)
            rec["compact_deliver_over_apply"] = round(q["compact_deliver"]["ms"] / q["apply"]["ms"], 4)
            iqr = lambda a: q[a]["ms_q75"] - q[a]["ms_q25"]  # noqa: E731
            rec["deliver_slower_than_apply_beyond_spread"] = bool(
                q["deliver"]["ms"] - q["apply"]["ms"] > iqr("deliver") + iqr("apply"))
            rec["agree"] = bool(agree)
            emit(rec)
            del stream, state0
        del orig, pieces, outs
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
