"""Inverted searches (XSG_FLAG_INVERT) next to the plain ones: whole synchronous calls on a resident shard built as
bench.py builds its corpus (16 MiB chunks replicated from seeded text templates).

    python scripts/invert_speed.py [--gib 10] [--templates 16] [--out profiles/invert_speed.jsonl]
    python scripts/invert_speed.py --baseline       # the plain COUNT_LINES | WITH_NEWLINES call alone, five repeats
    python scripts/invert_speed.py --trace          # one call of each kind and nothing else, for a kernel trace

One JSON line per (needle, call), appended to --out: ms of the first call and the mean of three more.  `Sherlock` is
rare (the inverted result is nearly every line of the shard), `e` is in most lines (the inverted result is small).
--baseline runs on any build of the library (XSG_LIB selects one): the inverted count is that pass plus one small
kernel, so its spread over five repeats on the commit before the flag is the margin the inverted count is held to.
--trace is meant for  rocprofv3 --kernel-trace --stats -- python scripts/invert_speed.py --trace : the complement
stage's kernels (k_invert_bounds, k_invert_tile<false>, k_invert_tile<true>) next to one k_scan count pass.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "oracle")]

import corpus  # noqa: E402
import xsg  # noqa: E402

NEEDLES = [b"Sherlock", b"e"]
INVERT = getattr(xsg, "FLAG_INVERT", 0)


def build_shard(args):
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
    return shard_t, ctx, shard, int(ln.sum())


def search_n(shard, mode):
    """xsg_search alone: the result stays where the search left it (fetching 3 GB of offsets into pageable memory would
    time the copy, not the search)"""
    n = C.c_uint64(0)
    xsg._check(shard._lib.xsg_search(shard.h, mode, C.byref(n)))
    return n.value


def timed(fn, repeats=3):
    t0 = time.perf_counter()
    got = fn()
    first = (time.perf_counter() - t0) * 1e3
    each = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        assert fn() == got
        each.append((time.perf_counter() - t0) * 1e3)
    return got, first, each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=10.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "invert_speed.jsonl"))
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    keep, ctx, shard, total = build_shard(args)

    def emit(row):
        row.update({"gib": round(total / 2**30, 2), "label": args.label})
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    if args.trace:
        ctx.set_pattern(b"Sherlock")
        shard.count(xsg.COUNT_MATCHES)                      # one k_scan count pass
        search_n(shard, xsg.LINE_BYTE_OFFSETS)              # the plain launch sequence
        ctx.set_pattern(b"Sherlock", INVERT)
        search_n(shard, xsg.LINE_BYTE_OFFSETS)              # ... and the inverted one: the same, then the complement stage
        shard.count(xsg.COUNT_LINES)
        return
    if args.baseline:
        for pat in NEEDLES:
            ctx.set_pattern(pat)
            mode = xsg.COUNT_LINES | xsg.WITH_NEWLINES
            got, first, each = timed(lambda: int(shard.count(mode)[xsg.CTR_LINES]), repeats=5)
            emit({"needle": pat.decode(), "call": "count_lines|newlines", "invert": False, "result": got, "first_ms": round(first, 3),
                  "ms_each": [round(x, 3) for x in each], "ms": round(sum(each) / len(each), 3),
                  "spread_ms": round(max(each) - min(each), 3)})
        return
    for pat in NEEDLES:
        for inv in (False, True):
            ctx.set_pattern(pat, INVERT if inv else 0)
            calls = [("count_lines", lambda: int(shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]), 5),
                     ("count_lines|newlines", lambda: int(shard.count(xsg.COUNT_LINES | xsg.WITH_NEWLINES)[xsg.CTR_LINES]), 5),
                     ("line_byte_offsets", lambda: search_n(shard, xsg.LINE_BYTE_OFFSETS), 3)]
            if inv and pat == b"e":
                calls.append(("lines", lambda: search_n(shard, xsg.LINES), 3))
            for name, fn, reps in calls:
                got, first, each = timed(fn, reps)
                emit({"needle": pat.decode(), "call": name, "invert": inv, "result": got, "first_ms": round(first, 3),
                      "ms_each": [round(x, 3) for x in each], "ms": round(sum(each) / len(each), 3),
                      "spread_ms": round(max(each) - min(each), 3), "kernel": shard.scan_kernel_name(xsg.COUNT_LINES if name.startswith("count") else xsg.LINE_BYTE_OFFSETS)})


if __name__ == "__main__":
    main()
