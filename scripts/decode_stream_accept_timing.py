#!/usr/bin/env python3
"""A decode stream's accept (rlnc_decode_stream_accept; include/rlnc_hip.h, "Decode streams") against its bandwidth
floor and against the routes a receiver had before it.  The arms alternate in one process; WARM warm-ups, then the median
and quartiles of TIMED repetitions (SLOW_TIMED for the loop of one copy per arrival).  One JSON line per (shape,
arrivals per object).  The arrivals are `per` pieces for every object, randomly interleaved, into empty objects.

  accept   (a) DecodeStream.accept: HIP events (`accept_ms`) and wall clock between two synchronisations.
  copy     (b) the floor: torch's device copy of the same number of bytes, contiguous to contiguous.  HIP events.
  move     (b') DecodeStream.compact on objects whose slot 0 is useless and whose next `per` slots are kept, so that its
           move launch shifts the same number of bytes by one slot with the same misaligned 16-byte accesses; the whole
           compaction is timed (its plan, rows and commit launches are 15-50 us: profiles/r16_stream_compact.jsonl).
           HIP events; the state is initialised and pushed again before every repetition, outside the timing.
  index    (c) the strongest route with the slots known on the host: the read-back of `answered` (a synchronisation), the
           slots computed with numpy, the indices uploaded and one index_copy_ into pieces.view(-1, k + L).  Wall clock.
  loop     (d) INTEGRATION.md's loop as printed: one copy_ per arrival with filled[] on the host.  Wall clock.

    python scripts/decode_stream_accept_timing.py profiles/r21_stream_accept.jsonl
    # the serial base launch at n = 1,024, 65,536 and 1,048,576 arrivals of 2 bytes over 256 objects, per launch from a
    # kernel trace of a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python scripts/decode_stream_accept_timing.py --base
    python scripts/decode_stream_accept_timing.py --base-from OUT/.../run_kernel_trace.csv >> profiles/r21_stream_accept.jsonl
    # one call per shape for a kernel trace of its own
    python scripts/decode_stream_accept_timing.py --shape 0 --per 8 --arm accept
    python3 scripts/profiles_index.py > profiles/INDEX.md     # the record's entry in the index
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.large_generation_timing import quart  # noqa: E402

WARM, TIMED, SLOW_TIMED = 3, 25, 3
# (objects, k, m, L)
SHAPES = [(64, 32, 40, 1 << 20), (64, 128, 136, 65536), (4096, 16, 24, 4096)]
PER = (1, 8)
BASE_N = (1024, 65536, 1 << 20)
BASE_WARM, BASE_TIMED = 1, 5
ARMS = ("accept", "copy", "move", "index", "loop")


def base_from_trace(path):
    """One JSON line per n of BASE_N from the kernel trace of a --base run: the three launches of the timed calls."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {"rank": [], "base": [], "move": []}
    for r in rows:
        for key in per:
            if "gf_stream_accept_" + key in r["Kernel_Name"]:
                per[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    calls = BASE_WARM + BASE_TIMED
    assert all(len(v) == calls * len(BASE_N) for v in per.values()), {k: len(v) for k, v in per.items()}
    for i, n in enumerate(BASE_N):
        rec = {"shape": "base launch: 256 objects, m 8192, k + L = 2", "arrivals": n, "steps": -(-n // 1024),
               "timed": "rocprofv3 --kernel-trace, per launch, median of %d calls after %d warm-up (us)" % (BASE_TIMED, BASE_WARM)}
        for key, v in per.items():
            ts = v[i * calls + BASE_WARM: (i + 1) * calls]
            rec[key + "_us"] = round(float(np.median(ts)), 2)
        rec["base_us_per_step"] = round(rec["base_us"] / rec["steps"], 3)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--per", type=int, default=None, help="that number of arrivals per object alone")
    ap.add_argument("--arm", default=None, choices=ARMS, help="that arm alone (for a trace)")
    ap.add_argument("--base", action="store_true", help="the calls of the base-launch measurement, for a kernel trace")
    ap.add_argument("--base-from", default=None, help="a kernel trace of a --base run: prints its JSON lines")
    args = ap.parse_args()
    if args.base_from:
        return base_from_trace(args.base_from)

    import torch

    import rlnc_amd
    from rlnc_amd import batch

    ctx = rlnc_amd.Context(0)
    ctx.set_rank_mode(1)

    if args.base:
        nobj, m = 256, 8192
        s = batch.DecodeStream(1, m, nobj, ctx)
        pieces = torch.zeros((nobj, m, 2), dtype=torch.uint8, device="cuda")
        for n in BASE_N:
            ids = torch.randint(0, nobj, (n,), dtype=torch.int32, device="cuda")
            arr = torch.randint(0, 256, (n, 2), dtype=torch.uint8, device="cuda")
            avail = torch.zeros(nobj, dtype=torch.int32, device="cuda")
            for _ in range(BASE_WARM + BASE_TIMED):
                avail.zero_()
                s.accept(arr, ids, pieces, avail)
                torch.cuda.synchronize()
        return

    shapes = SHAPES if args.shape is None else [SHAPES[args.shape]]
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")

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

    for nobj, k, m, L in shapes:
        S = k + L
        for per in (PER if args.per is None else (args.per,)):
            n = nobj * per
            rng = np.random.default_rng(per + k)
            ids_h = np.repeat(np.arange(nobj, dtype=np.int32), per)
            rng.shuffle(ids_h)
            ids = torch.from_numpy(ids_h).cuda()
            arrivals = torch.randint(0, 256, (n, S), dtype=torch.uint8, device="cuda")
            pieces = torch.zeros((nobj, m, S), dtype=torch.uint8, device="cuda")
            flat = torch.empty((n, S), dtype=torch.uint8, device="cuda")
            avail = torch.zeros(nobj, dtype=torch.int32, device="cuda")
            answered = torch.zeros(nobj, dtype=torch.int32, device="cuda")
            stream = batch.DecodeStream(k, m, nobj, ctx)
            stream.accept_reserve(n)
            # the compaction arm: slot 0 zero, slots 1 .. per the unit vectors, so that per pieces move by one slot
            mover = batch.DecodeStream(k, m, nobj, ctx)
            m_pieces = torch.randint(0, 256, (nobj, m, S), dtype=torch.uint8, device="cuda")
            hdr = torch.zeros((per + 1, k), dtype=torch.uint8, device="cuda")
            hdr[1:] = torch.eye(k, dtype=torch.uint8, device="cuda")[:per]
            m_avail = torch.full((nobj,), per + 1, dtype=torch.int32, device="cuda")
            m_rank = torch.zeros(nobj, dtype=torch.int32, device="cuda")

            def accept():
                stream.accept(arrivals, ids, pieces, avail)

            def copy():
                flat.copy_(arrivals)

            def move_setup():
                m_pieces[:, : per + 1, :k] = hdr
                ctx.lib.rlnc_decode_stream_init(ctx.h, mover.state.data_ptr(), mover.state.numel(), k, m, nobj)
                mover.push(m_pieces, m_avail, None, m_rank)

            def move():
                mover.compact(m_pieces)

            def index():
                filled = np.asarray(answered.tolist())  # the read-back: a synchronisation
                order = np.argsort(ids_h, kind="stable")
                sid = ids_h[order]
                start = np.concatenate([[0], np.cumsum(np.bincount(sid, minlength=nobj))[:-1]])
                slot = np.empty(n, np.int64)
                slot[order] = filled[sid] + np.arange(n) - start[sid]
                idx = torch.from_numpy(ids_h.astype(np.int64) * m + slot).cuda()
                pieces.view(-1, S).index_copy_(0, idx, arrivals)

            def loop():
                filled = answered.tolist()
                for i, o in enumerate(ids_h.tolist()):
                    pieces[o, filled[o]].copy_(arrivals[i], non_blocking=True)
                    filled[o] += 1
                avail.copy_(torch.tensor(filled, dtype=torch.int32))

            arms = {"accept": accept, "copy": copy, "move": move, "index": index, "loop": loop}
            if args.arm is not None:
                arms = {args.arm: arms[args.arm]}
            ev = {a: [] for a in arms}
            wl = {a: [] for a in arms}
            for it in range(WARM + TIMED):
                for a, fn in arms.items():
                    avail.zero_()
                    if a in ("index", "loop"):
                        if a == "index" or it < WARM + SLOW_TIMED:
                            t = wall_ms(fn)
                            if it >= WARM:
                                wl[a].append(t)
                        continue
                    if a == "move":
                        move_setup()
                    t = event_ms(fn)
                    if it >= WARM:
                        ev[a].append(t)
                    if a == "accept":
                        avail.zero_()
                        w = wall_ms(fn)
                        if it >= WARM:
                            wl[a].append(w)
            rec = {"shape": f"k{k} m{m} x{nobj} L{L}", "objects": nobj, "k": k, "m": m, "L": L, "per_object": per,
                   "arrivals": n, "bytes": n * S,
                   "timed": "arms interleaved; HIP events (ms) and wall clock between synchronisations (wall_ms), median "
                            "of %d (loop: %d)" % (TIMED, SLOW_TIMED)}
            for a in arms:
                if ev[a]:
                    q = quart(ev[a])
                    rec[a + "_ms"], rec[a + "_ms_q25"], rec[a + "_ms_q75"] = q["ms"], q["ms_q25"], q["ms_q75"]
                if wl[a]:
                    q = quart(wl[a])
                    rec[a + "_wall_ms"], rec[a + "_wall_ms_q25"], rec[a + "_wall_ms_q75"] = q["ms"], q["ms_q25"], q["ms_q75"]
            if args.arm is None:
                rec["accept_over_copy"] = round(rec["accept_ms"] / rec["copy_ms"], 4)
                rec["move_over_copy"] = round(rec["move_ms"] / rec["copy_ms"], 4)
                rec["index_over_accept_wall"] = round(rec["index_wall_ms"] / rec["accept_wall_ms"], 4)
                rec["loop_over_accept_wall"] = round(rec["loop_wall_ms"] / rec["accept_wall_ms"], 4)
                rec["copy_gb_s"] = round(n * S / rec["copy_ms"] / 1e6, 1)
                # every arm leaves the same pieces: accept last, against the index route
                avail.zero_()
                index()
                want = pieces.clone()
                pieces.zero_()
                accept()
                rec["agree"] = bool(torch.equal(pieces, want)) and bool((avail == per).all())
                assert bool((m_rank == per).all())
            emit(rec)
            del arrivals, pieces, flat, m_pieces, stream, mover
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
