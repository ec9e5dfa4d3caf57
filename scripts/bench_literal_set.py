"""A literal list next to the regex route that stood in for it: whole synchronous calls on a resident shard built as
bench.py builds its corpus (16 MiB chunks replicated from seeded corpus.py templates).

    python scripts/bench_literal_set.py [--gib 2] [--templates 16] [--regex-only] [--list-flags N] [--label NAME] [--out FILE]

For (Sherlock, Holmes), an 8-word list and a 300-word list it times xsg_count(XSG_COUNT_LINES) and an XSG_LINES search
through xsg_set_literals; for the first two also the same search through XSG_FLAG_REGEX with E(S) = l1|l2|...  One warm-up
call, then 5 repetitions: the median, the minimum and the maximum in ms.  `kernel_ms` is the candidate count pass alone
(xsg_time_scan_kernel) and `kernel_share` its part of the median count call.  One JSON line per (list, route, tag), appended
to --out if given.  --regex-only times the regex route alone: run it with XSG_LIB pointing at a build of the parent commit
for the yardstick (that library has no xsg_set_literals).  --list-flags N sets the lists through xsg_set_literals_opts(..., N)
(1: XSG_LIST_WHOLE_WORDS; the regex route has no such option and is left out); every row says which it ran with."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "x-search_amd")]

import corpus  # noqa: E402
import xsg  # noqa: E402

REPS = 5


def lists():
    rng = np.random.Generator(np.random.PCG64(300))
    made = [bytes(rng.integers(97, 123, size=int(rng.integers(4, 11))).astype(np.uint8)) for _ in range(292)]
    eight = [b"Sherlock", b"Holmes", b"Watson", b"detective", b"street", b"locked", b"which", b"their"]
    return [("2-words", [b"Sherlock", b"Holmes"]), ("8-words", eight), ("300-words", eight + made)]


def timed(call):
    call()  # warm-up
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return r, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--regex-only", action="store_true")
    ap.add_argument("--list-flags", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
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
    sink = open(args.out, "a") if args.out else None

    def report(name, route, tag, result, ms, extra):
        med = statistics.median(ms)
        row = {"label": args.label, "list": name, "route": route, "tag": tag, "result": int(result), "median_ms": round(med, 3),
               "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "gbs": round(total / med / 1e6, 1),
               "gib": round(total / 2**30, 2), "reps": REPS, "list_flags": args.list_flags}
        row.update(extra)
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for name, lits in lists():
        routes = []
        if not args.regex_only:
            routes.append(("list", lambda lits=lits: ctx.set_literals(xsg.literal_list(lits), 0, args.list_flags)))
        if len(lits) <= 8 and not args.list_flags:
            routes.append(("regex", lambda lits=lits: ctx.set_pattern(b"|".join(lits), xsg.FLAG_REGEX)))
        for route, set_it in routes:
            set_it()
            lines, ms = timed(lambda: int(shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]))
            kernel = shard.time_scan_kernel(xsg.COUNT_LINES, 5)
            report(name, route, "count_lines", lines, ms,
                   {"kernel_ms": round(kernel, 3), "kernel_share": round(kernel / statistics.median(ms), 3),
                    "kernel": shard.scan_kernel_name(xsg.COUNT_LINES)})
            n, ms = timed(lambda: int(shard.search_lines_view()[0].size))
            assert n == lines or n == lines - 1  # (a last line without its newline is counted, not handed out)
            report(name, route, "lines", n, ms, {})


if __name__ == "__main__":
    main()
