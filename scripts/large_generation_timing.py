#!/usr/bin/env python3
"""Rank mode 1 beyond LDS: the workspace-resident true-rank elimination (rank_large.hip, decode paths 7 and 8) against
what the library did before it, on identical pieces.  Every configuration alternates with its counterpart on one
context, 3 warm-ups, then the median and quartiles of 25 timed calls.  One JSON line per (row, shape, path); `agree` =
the outputs of the two paths of a row are identical.

  rank_lds    decode_batch_eliminate, HIP events around the call: path 8 against path 0 (rank.hip) where both apply --
              the price of keeping the state in HBM / L2 instead of LDS.  agree: T, statuses, ranks.
  host        path 7 against path 1 (host threads' elimination, what path 0 does beyond LDS), dense and density 4:
              `wall_ms` is the synchronous decode_batch (L = 16, so the elimination is nearly all of it) under each
              path; the path-7 line also carries `elim_ms`, HIP events around decode_batch_eliminate alone.
              agree: piece statuses, object statuses, lengths and decoded payloads.
  whole_call  decode_batch_device of 4 x k = 1,024 x 32 KiB under path 7, HIP events, beside `elim_ms` of the same
              pieces: the elimination's share of the call next to the T x data product.

Which path to prefer (one MI355X, profiles/r09_large_generation.jsonl).  Where rank.hip applies, path 7 keeps it; path
8 there is for tests and A/Bs -- it lost at the bench's 32 x k = 32 (0.093 against 0.158 ms: four launches for one
block) and won at 1 x k = 200, m = 210 (3.84 against 1.32 ms: one workgroup against many), a single-object result that
does not carry to batches.  Beyond LDS, path 7 against the host elimination, synchronous call against synchronous call:
1.95x at 4 x k = 1,024 dense, 1.66x at 64 x k = 256 dense, 1.1-1.3x at 16 x k = 512 dense and at density 4 of k = 256 and
k = 1,024, and 0.85x at 16 x k = 512 with density 4 -- sixteen sparse mid-sized objects, one vectorised host thread each,
are the host's.  So: path 7 for k of about 1,000 and more, for anything that must stay stream-ordered or be captured,
and when the host threads are busy; path 0 or 1 for batches of many sparse objects of a few hundred pieces when a
synchronous call is acceptable.  At 4 x k = 1,024 x 32 KiB the elimination is 0.90 of the whole decode_batch_device.

    python scripts/large_generation_timing.py [out.jsonl]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, TIMED = 3, 25
RANK_LDS = [("k200 m210 x1 dense", 1, 200, 210, 0), ("bench k32 x32 dense", 32, 32, 32, 0)]
HOST = [(f"k{k} m{k + 8} x{n} {'dense' if d == 0 else 'density %d' % d}", n, k, k + 8, d)
        for n, k in ((64, 256), (16, 512), (4, 1024)) for d in (0, 4)]
WHOLE = ("k1024 m1032 x4 dense, 32 KiB pieces", 4, 1024, 1032, 32768)


def coefficients(rng, n, k, m, density):
    if density == 0:
        return rng.integers(0, 256, (n, m, k), dtype=np.uint8)
    co = np.zeros((n, m, k), np.uint8)
    for _ in range(density):
        co[np.arange(n)[:, None], np.arange(m)[None, :], rng.integers(0, k, (n, m))] = \
            rng.integers(1, 256, (n, m), dtype=np.uint8)
    return co


def quart(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"ms": round(float(q[1]), 4), "ms_q25": round(float(q[0]), 4), "ms_q75": round(float(q[2]), 4)}


def main():
    import torch

    import rlnc_amd
    from oracle import np_oracle as npo
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

    # ---- against rank.hip --------------------------------------------------------------------------------------------
    for name, n, k, m, density in RANK_LDS:
        co = coefficients(np.random.default_rng(k * 7 + m), n, k, m, density)
        pieces = torch.zeros((n, m, k + 16), dtype=torch.uint8, device="cuda")
        pieces[:, :, :k] = torch.from_numpy(co).cuda()
        bufs = {p: elim_bufs(n, k, m) for p in (0, 8)}
        ts = {0: [], 8: []}
        for it in range(WARM + TIMED):
            for p in (0, 8):
                ctx.set_decode_path(p)
                t = event_ms(lambda: batch.decode_batch_eliminate(pieces, k, *bufs[p], ctx))
                if it >= WARM:
                    ts[p].append(t)
        agree = all(torch.equal(x, y) for x, y in zip(bufs[0], bufs[8]))
        for p in (0, 8):
            emit({"row": "rank_lds", "shape": name, "objects": n, "k": k, "m": m, "decode_path": p,
                  "timed": "decode_batch_eliminate, HIP events", **quart(ts[p]),
                  "full_rank": int((bufs[p][2] == k).sum()), "agree": agree})

    # ---- against the host elimination -------------------------------------------------------------------------------
    L = 16
    for name, n, k, m, density in HOST:
        rng = np.random.default_rng(k * 11 + density)
        co = coefficients(rng, n, k, m, density)
        src = rng.integers(0, 256, (n, k, L), dtype=np.uint8)
        src[:, -1, -1] = 0x81  # a valid payload end
        pieces = torch.from_numpy(np.stack([npo.encode(src[o], co[o]) for o in range(n)])).cuda()
        eb = elim_bufs(n, k, m)
        dec = {p: torch.zeros((n, k, L), dtype=torch.uint8, device="cuda") for p in (1, 7)}
        res, wall, elim = {}, {1: [], 7: []}, []
        for it in range(WARM + TIMED):
            for p in (1, 7):
                ctx.set_decode_path(p)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[p] = batch.decode_batch(pieces, k, dec[p], ctx)
                t = (time.perf_counter() - t0) * 1e3
                if it >= WARM:
                    wall[p].append(t)
            t = event_ms(lambda: batch.decode_batch_eliminate(pieces, k, *eb, ctx))  # path 7 still set
            if it >= WARM:
                elim.append(t)
        agree = all(np.array_equal(x, y) for x, y in zip(res[1], res[7])) and torch.equal(dec[1], dec[7])
        for p in (1, 7):
            q = quart(wall[p])
            rec = {"row": "host", "shape": name, "objects": n, "k": k, "m": m, "density": density, "decode_path": p,
                   "timed": "decode_batch (synchronous), wall", "wall_ms": q["ms"], "wall_ms_q25": q["ms_q25"],
                   "wall_ms_q75": q["ms_q75"], "full_rank": int((eb[2] == k).sum()), "agree": agree}
            if p == 7:
                rec["elim_ms"] = quart(elim)["ms"]
                rec["host_wall_over_device_wall"] = round(quart(wall[1])["ms"] / q["ms"], 3)
            emit(rec)

    # ---- the whole device call ---------------------------------------------------------------------------------------
    name, n, k, m, L = WHOLE
    rng = np.random.default_rng(1024)
    co = torch.from_numpy(coefficients(rng, n, k, m, 0)).cuda()
    src = torch.from_numpy(rng.integers(0, 256, (n, k, L), dtype=np.uint8)).cuda()
    src[:, -1, -1] = 0x81
    pieces = torch.empty((n, m, k + L), dtype=torch.uint8, device="cuda")
    ctx.set_decode_path(0)
    batch.encode_batch(src, co, pieces, ctx)
    ctx.set_decode_path(7)
    eb = elim_bufs(n, k, m)
    decoded = torch.zeros((n, k, L), dtype=torch.uint8, device="cuda")
    outs = (torch.empty((n, m), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda"),
            torch.empty((n,), dtype=torch.int64, device="cuda"))
    whole, elim = [], []
    for it in range(WARM + TIMED):
        a = event_ms(lambda: batch.decode_batch_device(pieces, k, decoded, *outs, ctx))
        b = event_ms(lambda: batch.decode_batch_eliminate(pieces, k, *eb, ctx))
        if it >= WARM:
            whole.append(a)
            elim.append(b)
    agree = bool(torch.equal(decoded, src)) and bool((eb[2] == k).all()) and bool(torch.equal(eb[1], outs[0]))
    emit({"row": "whole_call", "shape": name, "objects": n, "k": k, "m": m, "L": L, "decode_path": 7,
          "timed": "decode_batch_device, HIP events", **quart(whole), "elim_ms": quart(elim)["ms"],
          "elim_share": round(quart(elim)["ms"] / quart(whole)["ms"], 3), "agree": agree})
    ctx.set_decode_path(0)
    if out:
        out.close()


if __name__ == "__main__":
    main()
