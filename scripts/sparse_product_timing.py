#!/usr/bin/env python3
"""Sparse product (sparse.hip: rlnc_encode_batch_sparse / rlnc_recode_batch_sparse) against the dense call on the
expanded coefficients (rlnc_encode_batch / rlnc_recode_batch, the default kernel variant), same input, same context:
HIP events on the launch stream around one call, the two paths alternating, median and quartiles of 25 timed calls
each after 3 warm-ups.  One JSON line per (shape, path); `agree` = both outputs are identical.  Each line carries
two byte counts of the shape -- gathered = n·w·width per object (the source bytes the sparse kernel reads), written =
n·(k + L) per object (n·width for a recode) -- and both divided by the median time, to be read against the device's
row-gather rates (16.8-18.8 TB/s from an XCD's L2, 5.5-5.8 TB/s from HBM).

    python scripts/sparse_product_timing.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KiB, MiB = 1024, 1024 * 1024
SHAPES = [  # kind, objects, k, L, n (encode: coded pieces; recode: received), count (recode), the w's
    ("encode", 32, 32, MiB, 64, 0, (2, 4, 8, 32)),
    ("encode", 8, 128, 256 * KiB, 128, 0, (2, 4, 8, 16)),
    ("encode", 4, 1024, 32 * KiB, 1024, 0, (4, 8, 16)),
    ("encode", 4096, 16, 4 * KiB, 16, 0, (2, 4)),
    ("recode", 1, 128, 64 * KiB, 64, 64, (4,)),
]
WARMUP, TIMED = 3, 25


def main():
    import torch

    import rlnc_amd
    from rlnc_amd import batch, sparse

    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    ctx = rlnc_amd.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(8)
    for kind, B, k, L, n, count, ws in SHAPES:
        full = k + L
        if kind == "encode":
            n_in, n_out, width = k, n, L
            inp = torch.randint(0, 256, (B, k, L), dtype=torch.uint8, device="cuda", generator=gen)
        else:
            n_in, n_out, width = n, count, full
            inp = torch.randint(0, 256, (B, n, full), dtype=torch.uint8, device="cuda", generator=gen)
        outs = {p: torch.empty((B, n_out, full), dtype=torch.uint8, device="cuda") for p in ("sparse", "dense")}
        for w in ws:
            rng = np.random.default_rng(k * 31 + w)
            ent = [sparse.draw(rng, n_out, n_in, w) for _ in range(B)]
            idx, val = np.stack([e[0] for e in ent]), np.stack([e[1] for e in ent])
            didx, dval = torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda()
            dco = torch.from_numpy(sparse.to_dense(idx, val, n_in)).cuda()

            def call(path):
                if kind == "encode":
                    if path == "sparse":
                        batch.encode_batch_sparse(inp, didx, dval, outs[path], ctx)
                    else:
                        batch.encode_batch(inp, dco, outs[path], ctx)
                elif path == "sparse":
                    batch.recode_batch_sparse(inp, didx, dval, outs[path], k, ctx)
                else:
                    batch.recode_batch(inp, dco, outs[path], k, ctx)

            ts = {"sparse": [], "dense": []}
            for it in range(WARMUP + TIMED):
                for path in ("sparse", "dense"):
                    a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call(path)
                    b_.record()
                    torch.cuda.synchronize()
                    if it >= WARMUP:
                        ts[path].append(a.elapsed_time(b_))
            agree = bool(torch.equal(outs["sparse"], outs["dense"]))
            gathered, written = B * n_out * w * width, B * n_out * full
            for path in ("sparse", "dense"):
                q = np.percentile(ts[path], [25, 50, 75])
                sec = float(q[1]) * 1e-3
                rec = {"kind": kind, "objects": B, "k": k, "L": L, "n": n, "count": count, "w": w, "path": path,
                       "ms": round(float(q[1]), 4), "ms_q25": round(float(q[0]), 4), "ms_q75": round(float(q[2]), 4),
                       "gathered_bytes": gathered, "written_bytes": written,
                       "gathered_TBps": round(gathered / sec / 1e12, 3), "written_TBps": round(written / sec / 1e12, 3),
                       "agree": agree}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
            del didx, dval, dco
        del inp, outs
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
