"""Line-anchored regexes next to their bodies: whole synchronous xsg_count calls (COUNT_MATCHES, COUNT_LINES) on a
resident shard built as bench.py builds its corpus (16 MiB chunks replicated from seeded text templates).

    python scripts/anchor_speed.py [--gib 10] [--templates 16] [--anchored-only]

Prints one JSON line per (expression, mode): ms of the first call and the mean of three more, and the kernel name.
The first call of a pattern on a binding is the comparable figure: later calls of a factor-prefiltered expression
reuse the tile marks of the first, which no other route caches.  (XSG_RX_FAC=0 in the environment switches the
factor prefilter off: run with --anchored-only for the anchored walks on their own.)
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "oracle")]

import corpus  # noqa: E402
import xsg  # noqa: E402

PAIRS = [("(?m)^Sherlock", "Sherlock"), ("(?m)Holmes[.,]$", "Holmes[.,]"), ("(?m)^Sher.*mes", "Sher.*mes"),
         ("(?m)\\w+ing$", "\\w+ing")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=10.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--anchored-only", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    blocks = [corpus.text_block(args.seed, i, (16 << 20) + 1 + corpus._mix(args.seed, 1000 + i) % 61)
              for i in range(args.templates)]
    nchunks = int(round(args.gib * 2**30 / (16 << 20)))
    plan = np.array([corpus._mix(args.seed ^ 0xC0FFEE, c) % args.templates for c in range(nchunks)])
    off, ln, cap = corpus.chunk_table(np.array([blocks[p].size for p in plan]))
    shard_t = torch.empty(cap, dtype=torch.uint8, device=dev)
    dev_t = [torch.from_numpy(b).to(dev) for b in blocks]
    for c in range(nchunks):
        shard_t[int(off[c]):int(off[c]) + int(ln[c])].copy_(dev_t[int(plan[c])])
    torch.cuda.synchronize()
    del dev_t
    ctx = xsg.Context(0)
    ctx.set_pattern(b"x")
    shard = xsg.Shard(ctx, shard_t.data_ptr(), cap, xsg.make_chunks(off, ln))
    total = int(ln.sum())
    for anchored, body in PAIRS:
        for expr in (anchored,) if args.anchored_only else (anchored, body):
            for mode, ctr, name in ((xsg.COUNT_MATCHES, xsg.CTR_MATCHES, "count_matches"),
                                    (xsg.COUNT_LINES, xsg.CTR_LINES, "count_lines")):
                ctx.set_pattern(expr.encode(), xsg.FLAG_REGEX)
                t0 = time.perf_counter()
                got = int(shard.count(mode)[ctr])
                first = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                for _ in range(3):
                    assert int(shard.count(mode)[ctr]) == got
                ms = (time.perf_counter() - t0) / 3 * 1e3
                print(json.dumps({"expr": expr, "mode": name, "result": got, "first_ms": round(first, 2),
                                  "ms": round(ms, 2), "gbs": round(total / ms / 1e6, 1), "gib": round(total / 2**30, 2),
                                  "xsg_rx_fac": os.environ.get("XSG_RX_FAC", ""),
                                  "kernel": shard.scan_kernel_name(mode)}), flush=True)


if __name__ == "__main__":
    main()
