#!/usr/bin/env python3
"""A decode stream's compaction (rlnc_decode_stream_compact; include/rlnc_hip.h, "Decode streams") against what a
receiver could do without it, on identical streams.  The arms alternate on one context, HIP events around each; WARM
warm-ups, then the median and quartiles of TIMED repetitions.  Before every arm the pieces and the state are restored
(not timed) to what one push of `done` slots left.  One JSON line per (shape, useless share, placement).

  compact     rlnc_decode_stream_compact with the pieces: plan, row gather, piece move, commit.
  state_only  the same call without pieces (three launches); move_ms = compact - state_only is the piece move's share.
  repush      the only alternative before the call existed: snapshot the statuses, synchronise, pick the useful slots on
              the host, gather those pieces with torch into the first slots, rlnc_decode_stream_init, and push
              (eliminate) all of them again.  The events span the synchronisation and the host's decision.
  copy        the yardstick of the move: a plain torch device copy of as many bytes as the move copies (the kept pieces
              that change slot, k + L bytes each).

`move_over_copy` = copy_ms / move_ms; `move_hbm_share` = the move's traffic (every byte read once and written once) over
8 TB/s.  `agree` = the compact arm and the repush arm end with identical snapshots (T, statuses, ranks) and identical
kept pieces.

A stream of m slots has `done` of them pushed, `useless` of which are useless (a zero piece before the first useful one,
else a duplicate of it), the others independent: a quarter or three quarters useless, first = the useless slots come
first, interleaved = spread evenly.  The useful slots cannot outnumber k, so at a quarter useless done = min(m, 4k/3
rounded down to a multiple of 4).

    python scripts/decode_stream_compact_timing.py profiles/r16_stream_compact.jsonl
    python3 scripts/profiles_index.py > profiles/INDEX.md     # the record's entry in the index
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.large_generation_timing import quart  # noqa: E402

WARM, TIMED = 3, 25
HBM_PEAK = 8e12
# (objects, k, m, L)
SHAPES = [(32, 32, 64, 1 << 20), (4096, 16, 24, 4096), (64, 256, 264, 65536)]
SHARES = ((1, 4), (3, 4))
PLACEMENTS = ("first", "interleaved")


def vectors(rng, k, done, useless, placement):
    """co [done][k] and the useful slots: independent (triangular) useful vectors, `useless` useless ones."""
    if placement == "first":
        bad = set(range(useless))
    else:
        bad = {t for t in range(done) if (t + 1) * useless // done > t * useless // done}
    assert len(bad) == useless
    co = np.zeros((done, k), np.uint8)
    useful = []
    for t in range(done):
        if t in bad:
            if useful:
                co[t] = co[useful[0]]
            continue
        i = len(useful)
        co[t, :i] = rng.integers(0, 256, i)
        co[t, i] = rng.integers(1, 256)
        useful.append(t)
    return co, useful


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch
    from rlnc_amd.errors import check

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

    def snap_bufs(n, k, m):
        return (torch.empty((n, k, m), dtype=torch.uint8, device="cuda"),
                torch.empty((n, m), dtype=torch.int32, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"))

    for n, k, m, L in SHAPES:
        S = k + L
        orig = torch.randint(0, 256, (n, m, S), dtype=torch.uint8, device="cuda")
        pieces = torch.empty_like(orig)
        for num, den in SHARES:
            done = m if num * 4 > den * 2 else min(m, (4 * k // 3) & ~3)
            useless = done * num // den
            for placement in PLACEMENTS:
                co, useful = vectors(np.random.default_rng(k + num), k, done, useless, placement)
                assert len(useful) == done - useless <= k
                r = len(useful)
                orig[:, :done, :k] = torch.from_numpy(co).cuda()
                moved = sum(1 for j, u in enumerate(useful) if u != j)
                move_bytes = n * moved * S
                stream, again = batch.DecodeStream(k, m, n, ctx), batch.DecodeStream(k, m, n, ctx)
                stream.push(orig, torch.full((n,), done, dtype=torch.int32, device="cuda"))
                state0 = stream.state.clone()
                kept = torch.empty((n, k), dtype=torch.int32, device="cuda")
                ans = torch.empty((n,), dtype=torch.int32, device="cuda")
                snaps = {"compact": snap_bufs(n, k, m), "repush": snap_bufs(n, k, m)}
                stream.snapshot(*snaps["compact"])
                assert bool((snaps["compact"][2] == r).all())
                copy_src = orig.view(-1)[:max(move_bytes, 1)]
                copy_dst = torch.empty(max(move_bytes, 1), dtype=torch.uint8, device="cuda")
                avail = torch.empty((n,), dtype=torch.int32, device="cuda")
                results = {}

                def restore(s):
                    pieces.copy_(orig)
                    s.state.copy_(state0)

                def repush():
                    ps = snaps["repush"][1]
                    again.snapshot(piece_status=ps)
                    st = ps.cpu().numpy()  # synchronises
                    idx = np.zeros((n, k), np.int64)
                    cnt = np.zeros(n, np.int32)
                    for o in range(n):
                        u = np.flatnonzero(st[o] == 0)
                        idx[o, :u.size] = u
                        cnt[o] = u.size
                    most = int(cnt.max())
                    sel = torch.from_numpy(idx[:, :most]).cuda()
                    gathered = torch.gather(pieces, 1, sel[:, :, None].expand(n, most, S))
                    pieces[:, :most] = gathered
                    avail.copy_(torch.from_numpy(cnt))
                    check(ctx.lib.rlnc_decode_stream_init(ctx.h, C.c_void_p(again.state.data_ptr()),
                                                          again.state.numel(), k, m, n), ctx.lib)
                    again.push(pieces, avail)

                arms = {
                    "compact": (stream, lambda: stream.compact(pieces, None, kept, ans)),
                    "state_only": (stream, lambda: stream.compact(None, None, kept, ans)),
                    "repush": (again, repush),
                    "copy": (stream, lambda: copy_dst.copy_(copy_src)),
                }
                ts = {a: [] for a in arms}
                for it in range(WARM + TIMED):
                    for a, (s, fn) in arms.items():
                        restore(s)
                        t = event_ms(fn)
                        if it >= WARM:
                            ts[a].append(t)
                        if it == WARM + TIMED - 1 and a in snaps:
                            s.snapshot(*snaps[a])
                            results[a] = pieces[:, :r].clone()
                agree = all(torch.equal(x, y) for x, y in zip(snaps["compact"], snaps["repush"])) and \
                    torch.equal(results["compact"], results["repush"])
                q = {a: quart(v) for a, v in ts.items()}
                move_ms = q["compact"]["ms"] - q["state_only"]["ms"]
                rec = {"shape": f"k{k} m{m} x{n} L{L}", "objects": n, "k": k, "m": m, "L": L, "done": done,
                       "useless": useless, "useful": r, "placement": placement, "pieces_moved_per_object": moved,
                       "move_bytes": move_bytes,
                       "timed": "one call per arm on restored pieces and state, HIP events, median of %d" % TIMED}
                for a in arms:
                    rec[a + "_ms"], rec[a + "_ms_q25"], rec[a + "_ms_q75"] = q[a]["ms"], q[a]["ms_q25"], q[a]["ms_q75"]
                rec["move_ms"] = round(move_ms, 4)
                rec["repush_over_compact"] = round(q["repush"]["ms"] / q["compact"]["ms"], 2)
                if move_bytes and move_ms > 0:
                    rec["move_TBps_copied"] = round(move_bytes / (move_ms * 1e-3) / 1e12, 3)
                    rec["copy_TBps_copied"] = round(move_bytes / (q["copy"]["ms"] * 1e-3) / 1e12, 3)
                    rec["move_over_copy"] = round(q["copy"]["ms"] / move_ms, 3)
                    rec["move_hbm_share"] = round(2 * move_bytes / (move_ms * 1e-3) / HBM_PEAK, 3)
                rec["agree"] = bool(agree)
                emit(rec)
                del stream, again, state0, snaps, copy_dst
        del orig, pieces
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
