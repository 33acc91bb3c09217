#!/usr/bin/env python3
"""The sender's emit (rlnc_encode_emit; include/rlnc_hip.h) against its floor and against the only route a sender with
device-side counts had before it, on identical inputs.  The arms alternate on one context; WARM warm-ups, then the
median and quartiles of TIMED repetitions (ROUTE_TIMED for the host route, which is slow at many objects).  One JSON
line per (shape, want distribution).

  emit     EncodeEmitter.emit: the scan, the labels and headers, the block-address streams, the product of the program
           chosen by max_per_object and the perm product over the rest; want is read on the device.  HIP events
           (`emit_ms`) and wall clock between two synchronisations (`emit_wall_ms`).
  floor    (b) rlnc_encode_batch with one uniform n = the mean grant (rounded up), so the same total rows, with the
           counts known on the host and no packing: [obj][n][k+L].  HIP events.
  route    (c) what such a sender had to do before: read want back, synchronise, build one descriptor per emitting
           object on the host, rlnc_encode_ragged into per-object outputs, then gather the rows into the packed buffer
           (one index_select).  Wall clock between two synchronisations (it synchronises itself).

Want distributions: `all_k` every object k under max_per_object = k; `all_4` every object 4 under 4; `eighth_k` every
eighth object k and the rest 0, under k; `late_mix_cap8` / `late_mix_capk8` a late round's 1..5 per object under
max_per_object = 8 and = k + 8 (the cost of choosing the program by the cap); `all_zero` nothing to send: the idle
workgroups alone.  `agree` = after the last repetition emit's packets, ids and count equal the route's (and the
floor's rows where the split is uniform).

    python scripts/encode_emit_timing.py profiles/r22_encode_emit.jsonl
    python scripts/encode_emit_timing.py --shape 0 --dist all_k --arm emit     # one arm alone, for a kernel trace
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

from scripts.large_generation_timing import quart  # noqa: E402

WARM, TIMED, ROUTE_TIMED = 3, 25, 5
# (objects, k, L)
SHAPES = [(64, 32, 1 << 20), (64, 128, 65536), (4096, 16, 4096)]
DISTS = ("all_k", "all_4", "eighth_k", "late_mix_cap8", "late_mix_capk8", "all_zero")


def wants(dist, nobj, k, rng):
    """(want int32 [obj], max_per_object)"""
    if dist == "all_k":
        return np.full(nobj, k, np.int32), k
    if dist == "all_4":
        return np.full(nobj, 4, np.int32), 4
    if dist == "eighth_k":
        return np.where(np.arange(nobj) % 8 == 0, k, 0).astype(np.int32), k
    if dist.startswith("late_mix"):
        return rng.integers(1, 6, nobj).astype(np.int32), 8 if dist.endswith("cap8") else k + 8
    return np.zeros(nobj, np.int32), k


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--dist", default=None, choices=DISTS, help="that want distribution alone")
    ap.add_argument("--arm", default=None, choices=("emit", "floor", "route"), help="that arm alone (for a trace)")
    args = ap.parse_args()
    shapes = SHAPES if args.shape is None else [SHAPES[args.shape]]
    dists = DISTS if args.dist is None else (args.dist,)
    out_f = open(args.out, "w") if args.out else None

    def record(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")

    ctx = rlnc_amd.Context(0)

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

    for nobj, k, L in shapes:
        S = k + L
        src = torch.randint(0, 256, (nobj, k, L), dtype=torch.uint8, device="cuda")
        for dist in dists:
            want_h, cap = wants(dist, nobj, k, np.random.default_rng(k))
            w = np.clip(want_h, 0, cap)
            total = int(w.sum())
            n = max(total, nobj)  # the packet capacity: no truncation
            mean = -(-total // nobj) if total else 0
            want = torch.from_numpy(want_h).cuda()
            r = torch.randint(0, 256, (n, k), dtype=torch.uint8, device="cuda")
            o_emit = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
            ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            granted = torch.full((nobj,), -7, dtype=torch.int32, device="cuda")
            em = batch.EncodeEmitter(k, L, nobj, cap, n, ctx)
            o_route = torch.zeros((n, S), dtype=torch.uint8, device="cuda")
            scattered = torch.zeros((nobj, cap, S), dtype=torch.uint8, device="cuda")
            uniform = total > 0 and bool((w == mean).all())
            if mean:
                co = r[: nobj * mean].view(nobj, mean, k) if uniform else \
                    torch.randint(0, 256, (nobj, mean, k), dtype=torch.uint8, device="cuda")
                o_floor = torch.zeros((nobj, mean, S), dtype=torch.uint8, device="cuda")

            def emit():
                em.emit(src, want, r, o_emit, ids, count, granted)

            def floor():
                batch.encode_batch(src, co, o_floor, ctx)

            def route():
                wh = np.clip(want.cpu().numpy(), 0, cap)  # synchronises
                base = np.concatenate([[0], np.cumsum(wh)[:-1]])
                objs, rows = [], []
                for o in np.flatnonzero(wh):
                    b, g = int(base[o]), int(wh[o])
                    objs.append((src[o], r[b: b + g], scattered[o, :g]))
                    rows.append(o * cap + np.arange(g))
                if objs:
                    batch.encode_ragged(objs, ctx)
                    idx = torch.from_numpy(np.concatenate(rows)).cuda()
                    torch.index_select(scattered.view(nobj * cap, S), 0, idx, out=o_route[: len(idx)])

            arms = {"emit": emit, "route": route}
            if mean:
                arms["floor"] = floor
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
                    wt = wall_ms(fn)
                    if it >= WARM:
                        ev[a].append(t)
                        wl[a].append(wt)
            rec = {"shape": f"k{k} x{nobj} L{L}", "objects": nobj, "k": k, "L": L, "dist": dist, "max_per_object": cap,
                   "packets": total, "capacity": n, "floor_rows_per_object": mean,
                   "timed": "arms interleaved; HIP events (ms) and wall clock between synchronisations (wall_ms), "
                            "median of %d (route: wall clock only, %d)" % (TIMED, ROUTE_TIMED)}
            for a in arms:
                if ev[a]:
                    q = quart(ev[a])
                    rec[a + "_ms"], rec[a + "_ms_q25"], rec[a + "_ms_q75"] = q["ms"], q["ms_q25"], q["ms_q75"]
                q = quart(wl[a])
                rec[a + "_wall_ms"], rec[a + "_wall_ms_q25"], rec[a + "_wall_ms_q75"] = q["ms"], q["ms_q25"], q["ms_q75"]
            if args.arm is None:
                if mean:
                    rec["emit_over_floor"] = round(rec["emit_ms"] / rec["floor_ms"], 4)
                rec["route_over_emit_wall"] = round(rec["route_wall_ms"] / rec["emit_wall_ms"], 4)
                agree = int(count.item()) == total and torch.equal(o_emit[:total], o_route[:total])
                agree = agree and bool((ids[:total] == torch.from_numpy(np.repeat(np.arange(nobj), w)).cuda()).all())
                agree = agree and bool((ids[total:] == -1).all()) and bool((granted.cpu() == torch.from_numpy(w)).all())
                if uniform:
                    agree = agree and torch.equal(o_floor.view(-1, S), o_emit[:total])
                rec["agree"] = bool(agree)
            record(rec)
            del r, o_emit, o_route, scattered, em
            if mean:
                del co, o_floor
            torch.cuda.empty_cache()
        del src
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
