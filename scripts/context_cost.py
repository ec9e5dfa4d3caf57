"""What context lines cost: XSG_LINES and XSG_LINE_BYTE_OFFSETS with XSG_FLAG_CONTEXT(2, 2) next to the same calls with
(0, 0) on the exact list route (the route the widening stage sits on: the same calls on the parent commit), whole
synchronous calls at the C ABI on a resident shard built as bench.py builds its corpus, results taken where a caller reads
them without a copy (the shard's pinned buffers).

    python scripts/context_cost.py [--gib 10] [--templates 16] [--out profiles/context_cost.jsonl]

One JSON line per (pattern, tag, context), appended to --out: ms of the first call, of three more, the number of results
and the bytes the host receives; then one line per (pattern, tag) with the ratio context / plain.  `Sherlock` is the
sparse needle, `She` the needle in most lines.  XSG_LIST_FAST=0 keeps the (0, 0) calls on the exact route (the toggle
is re-read per call under XSG_TEST_HOOKS=1, set here before the library loads)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("XSG_TEST_HOOKS", "1")
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "oracle"), str(ROOT / "scripts")]

import xsg  # noqa: E402
from invert_speed import build_shard  # noqa: E402

PATTERNS = [(b"Sherlock", 0), (b"She", 0)]


def offsets_call(shard):
    n = C.c_uint64(0)
    xsg._check(shard._lib.xsg_search(shard.h, xsg.LINE_BYTE_OFFSETS, C.byref(n)))
    ptr, cnt = C.POINTER(C.c_uint64)(), C.c_uint64(0)
    xsg._check(shard._lib.xsg_result_u64_view(shard.h, C.byref(ptr), C.byref(cnt)))
    return cnt.value, 8 * cnt.value


def lines_call(shard):
    lens, data, offs = shard.search_lines_view()
    return int(lens.size), 16 * int(lens.size) + int(data.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=10.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--before", type=int, default=2)
    ap.add_argument("--after", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "context_cost.jsonl"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    keep, ctx, shard, total = build_shard(args)
    os.environ["XSG_LIST_FAST"] = "0"  # the baseline is the exact route
    with open(args.out, "a") as f:
        for pat, flags in PATTERNS:
            for tag, call in (("line_byte_offsets", offsets_call), ("lines", lines_call)):
                ms = {}
                for before, after in ((0, 0), (args.before, args.after)):
                    ctx.set_pattern(pat, flags | xsg.flag_context(before, after))
                    t0 = time.perf_counter()
                    n, nbytes = call(shard)
                    first = (time.perf_counter() - t0) * 1e3
                    each = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        assert call(shard) == (n, nbytes)
                        each.append((time.perf_counter() - t0) * 1e3)
                    ms[(before, after)] = sum(each) / len(each)
                    row = {"pattern": pat.decode(), "tag": tag, "context": [before, after], "route": "exact",
                           "gib": round(total / 2**30, 2), "results": n, "host_bytes": nbytes, "first_ms": round(first, 3),
                           "ms_each": [round(x, 3) for x in each], "ms": round(ms[(before, after)], 3), "label": args.label}
                    print(json.dumps(row), flush=True)
                    f.write(json.dumps(row) + "\n")
                ratio = {"pattern": pat.decode(), "tag": tag, "context": [args.before, args.after],
                         "ratio_to_plain": round(ms[(args.before, args.after)] / ms[(0, 0)], 3), "label": args.label}
                print(json.dumps(ratio), flush=True)
                f.write(json.dumps(ratio) + "\n")


if __name__ == "__main__":
    main()
