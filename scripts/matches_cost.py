"""What XSG_MATCHES costs next to XSG_MATCH_BYTE_OFFSETS of the same pattern: whole synchronous calls at the C ABI on a
resident shard built as bench.py builds its corpus (16 MiB chunks replicated from seeded text templates), results taken
where a caller reads them without a copy (xsg_result_u64_view / xsg_result_lines_view: the shard's pinned buffers).

    python scripts/matches_cost.py [--gib 10] [--templates 16] [--out profiles/matches_cost.jsonl]

One JSON line per (pattern, tag), appended to --out: ms of the first call, of three more, the number of results, the bytes
the host receives and the time the link alone needs for them at --link-gbs (57.1 GB/s device -> pinned on this pool,
DESIGN.md 3.4).  `Sherlock` is sparse, `\\w+ing` takes the automaton route (factor mask on a shard this size), `She` is the
dense case (a needle in most lines)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "oracle"), str(ROOT / "scripts")]

import xsg  # noqa: E402
from invert_speed import build_shard  # noqa: E402

PATTERNS = [(b"Sherlock", 0), (b"\\w+ing", xsg.FLAG_REGEX), (b"She", 0)]


def offsets_call(shard):
    n = C.c_uint64(0)
    xsg._check(shard._lib.xsg_search(shard.h, xsg.MATCH_BYTE_OFFSETS, C.byref(n)))
    ptr, cnt = C.POINTER(C.c_uint64)(), C.c_uint64(0)
    xsg._check(shard._lib.xsg_result_u64_view(shard.h, C.byref(ptr), C.byref(cnt)))
    return cnt.value, 8 * cnt.value


def matches_call(shard):
    lens, data, offs = shard.search_matches_view()
    return int(lens.size), 16 * int(lens.size) + int(data.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=10.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--link-gbs", type=float, default=57.1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "matches_cost.jsonl"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    keep, ctx, shard, total = build_shard(args)
    for pat, flags in PATTERNS:
        ctx.set_pattern(pat, flags)
        for tag, call in (("match_byte_offsets", offsets_call), ("matches", matches_call)):
            t0 = time.perf_counter()
            n, nbytes = call(shard)
            first = (time.perf_counter() - t0) * 1e3
            each = []
            for _ in range(3):
                t0 = time.perf_counter()
                assert call(shard) == (n, nbytes)
                each.append((time.perf_counter() - t0) * 1e3)
            row = {"pattern": pat.decode(), "tag": tag, "gib": round(total / 2**30, 2), "results": n, "host_bytes": nbytes,
                   "first_ms": round(first, 3), "ms_each": [round(x, 3) for x in each], "ms": round(sum(each) / len(each), 3),
                   "link_floor_ms": round(nbytes / (args.link_gbs * 1e9) * 1e3, 3), "label": args.label}
            line = json.dumps(row)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
