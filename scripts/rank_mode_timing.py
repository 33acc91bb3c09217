#!/usr/bin/env python3
"""Elimination launch time (rlnc_decode_batch_eliminate) in rank mode 1 (true rank, rank.hip) against rank mode 0
(the reference replica, rref.hip) on identical pieces: HIP events on the launch stream around one launch, the two
modes alternating on one context, median and quartiles of 25 timed launches each after 3 warm-ups.  Shapes: the
bench's decode shape (32 objects, k = m = 32), 4,096 objects of k = m = 16 dense, the sparse and dependent
4,096 x k = 16 shape of scripts/elim_timing.py (ELIM_SHAPES=small), density-2 sparse vectors, and two larger dense
shapes.  One JSON line per (shape, mode); `agree` = the two modes' statuses, ranks and T are identical.

    python scripts/rank_mode_timing.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # name, objects, k, m, zero fraction (or -density), dependent fraction
    ("bench k32 dense", 32, 32, 32, 0.0, 0.0),
    ("k16 x4096 dense", 4096, 16, 16, 0.0, 0.0),
    ("k16 m24 x4096 sparse 0.5 dep", 4096, 16, 24, 0.5, 0.1),
    ("k16 m48 x4096 density 2", 4096, 16, 48, -2, 0.0),
    ("k32 m64 x1024 density 3", 1024, 32, 64, -3, 0.0),
    ("k64 x64 dense", 64, 64, 64, 0.0, 0.0),
    ("k128 x512 dense", 512, 128, 128, 0.0, 0.0),
]


def coefficients(rng, B, k, m, sp, dep):
    if sp < 0:
        co = np.zeros((B, m, k), np.uint8)
        for _ in range(int(-sp)):
            co[np.arange(B)[:, None], np.arange(m)[None, :], rng.integers(0, k, (B, m))] = \
                rng.integers(1, 256, (B, m), dtype=np.uint8)
        return co
    co = rng.integers(0, 256, (B, m, k), dtype=np.uint8)
    co[rng.random((B, m, k)) < sp] = 0
    for o in range(B if dep > 0 else 0):
        for p in range(2, m):
            if rng.random() < dep:
                a, b = rng.integers(0, p, 2)
                co[o, p] = co[o, a] ^ co[o, b]
    return co


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    ctx = rlnc_amd.Context(0)
    L = 16  # the elimination reads only the coefficient bytes
    for name, B, k, m, sp, dep in SHAPES:
        rng = np.random.default_rng(k * 7 + m)
        co = coefficients(rng, B, k, m, sp, dep)
        pieces = torch.zeros((B, m, k + L), dtype=torch.uint8, device="cuda")
        pieces[:, :, :k] = torch.from_numpy(co).cuda()
        bufs = {mode: (torch.empty((B, k, m), dtype=torch.uint8, device="cuda"),
                       torch.empty((B, m), dtype=torch.int32, device="cuda"),
                       torch.empty((B,), dtype=torch.int32, device="cuda")) for mode in (0, 1)}
        ts = {0: [], 1: []}
        for it in range(28):
            for mode in (0, 1):
                ctx.set_rank_mode(mode)
                a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                batch.decode_batch_eliminate(pieces, k, *bufs[mode], ctx)
                b_.record()
                torch.cuda.synchronize()
                if it >= 3:
                    ts[mode].append(a.elapsed_time(b_))
        res = {mode: [t.cpu() for t in bufs[mode]] for mode in (0, 1)}
        agree = all(torch.equal(x, y) for x, y in zip(res[0], res[1]))
        same_status = bool(torch.equal(res[0][1], res[1][1]))
        for mode in (0, 1):
            q = np.percentile(ts[mode], [25, 50, 75])
            rec = {"shape": name, "objects": B, "k": k, "m": m, "rank_mode": mode, "ms": round(float(q[1]), 4),
                   "ms_q25": round(float(q[0]), 4), "ms_q75": round(float(q[2]), 4),
                   "full_rank": int((res[mode][2] == k).sum()), "objects_with_same_statuses":
                   int((res[0][1] == res[1][1]).all(dim=1).sum()), "agree": agree and same_status}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    ctx.set_rank_mode(0)
    if out:
        out.close()


if __name__ == "__main__":
    main()
