#!/usr/bin/env python3
"""What xsg_find_literals costs (profiles/literal_find_ab.jsonl, DESIGN.md sections 3.5i and 5).

2 GiB of resident corpus.py text (the buffer of scripts/literal_csr_cost.py) in 128 chunks of 16 MiB, under the 8-word
list and the 4096-literal list of literal_counts_cost.lists() (--lists; `dense e, th` is the list that makes every
eighth byte an occurrence).  Every leg is --runs interleaved runs (every other run in reverse order); a run = --calls
timed calls behind --warm untimed ones, its figure their median; a leg reports the median of its runs and their
min..max.  Device time, events round the stream-ordered forms on a stream of the caller's:
  find                       xsg_find_literals_async with cap_entries = total (read once, untimed, from a sizing call)
  find, sizing only          the same with cap_entries = 0: count pass, prefix sum and chunk_ptr -- no fill pass
  count_literals (floor)     xsg_count_literals_async: one scan
  two count passes (a)       two of them back to back on the same binding: the parent commit's kernel twice, the structural
                             floor of a size-then-fill design
and, on the host's clock because it waits and fetches (stream idle before, result in pinned memory after):
  search offsets (b)         xsg_search(XSG_MATCH_BYTE_OFFSETS) + xsg_result_u64_view of the same list under
                             XSG_FLAG_EXACT_TAIL: until now the only way to positions -- the winners of the leftmost-first
                             walk, without their literals
  find, synchronous          xsg_find_literals + xsg_result_literal_hits, for the same clock as (b)
Before any timing the result is checked for its form (chunk_ptr ascending from 0 to total, (pos, lit) strictly ascending
inside a chunk), its bincount against xsg_count_literals, two grids bit for bit, and the clipped call (cap = total - 1)
for its status word and the untouched entry at the capacity."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

os.environ["XSG_TEST_HOOKS"] = "1"  # the grid switch is re-read at every call
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "scripts")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--templates", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--lists", default="8-words,4096-distinct-grams")
    ap.add_argument("--grid", type=int, default=1024, help="the XSG_LITFIND_GRID value of the parity check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import corpus
    import literal_counts_cost
    import xsg
    dev = torch.device("cuda:0")
    blocks = [corpus.text_block(a.seed, i, (16 << 20) + 1 + corpus._mix(a.seed, 1000 + i) % 61) for i in range(a.templates)]
    nchunks = int(round(a.gib * 2**30 / (16 << 20)))
    plan = np.array([corpus._mix(a.seed ^ 0xC0FFEE, c) % a.templates for c in range(nchunks)])
    off, ln, cap = corpus.chunk_table(np.array([blocks[p].size for p in plan]))
    t = torch.empty(cap, dtype=torch.uint8, device=dev)
    dev_t = [torch.from_numpy(b).to(dev) for b in blocks]
    for c in range(nchunks):
        t[int(off[c]):int(off[c]) + int(ln[c])].copy_(dev_t[int(plan[c])])
    torch.cuda.synchronize()
    del dev_t
    named = dict(literal_counts_cost.lists())
    ctx = xsg.Context(0)
    ctx.set_pattern(b"x")
    n = int(len(ln))
    shard = xsg.Shard(ctx, t.data_ptr(), cap, xsg.make_chunks(off, ln))
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream != 0
    sink = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def device_ms(fn):
        for _ in range(a.warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def host_ms(fn):
        for _ in range(a.warm):
            fn()
        ms = []
        for _ in range(a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))

    def stats(v):
        return {"run_ms": [round(x, 4) for x in v], "ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def leg(name):
        lits = named[name]
        k = len(lits)
        ctx.set_literals(xsg.literal_list(lits), xsg.FLAG_EXACT_TAIL)
        d_cp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(1, dtype=torch.int64, device=dev)
        d_c = torch.empty(k, dtype=torch.int64, device=dev)
        none = torch.empty(8, dtype=torch.int64, device=dev)
        shard.find_literals_async(stream, d_cp.data_ptr(), n + 1, none.data_ptr(), none.data_ptr(), 0, d_st.data_ptr())  # the sizing pass
        torch.cuda.synchronize()
        total = int(d_cp[n].item())
        assert int(d_st.item()) == (xsg.STATUS_OVERFLOW if total else xsg.STATUS_OK)
        d_pos = torch.full((total + 1,), -1, dtype=torch.int64, device=dev)
        d_lit = torch.full((total + 1,), -1, dtype=torch.int32, device=dev)

        def find(cap_entries, grid=None):
            def call():
                if grid:
                    os.environ["XSG_LITFIND_GRID"] = str(grid)
                try:
                    shard.find_literals_async(stream, d_cp.data_ptr(), n + 1, d_pos.data_ptr(), d_lit.data_ptr(), cap_entries, d_st.data_ptr())
                finally:
                    os.environ.pop("XSG_LITFIND_GRID", None)
            return call

        def two_counts():
            shard.count_literals_async(stream, d_c.data_ptr(), k)
            shard.count_literals_async(stream, d_c.data_ptr(), k)

        # parity before any timing
        find(total)()
        torch.cuda.synchronize()
        assert int(d_st.item()) == xsg.STATUS_OK and int(d_cp[n].item()) == total and int(d_cp[0].item()) == 0
        assert int(d_pos[total].item()) == -1 and int(d_lit[total].item()) == -1, "an entry at the capacity was written"
        first = (d_cp.clone(), d_pos[:total].clone(), d_lit[:total].clone())
        if not bool((first[0][1:] >= first[0][:-1]).all()):
            raise SystemExit(f"PARITY FAILURE ({name}): chunk_ptr descends")
        if total:
            if int(first[2].min().item()) < 0 or int(first[2].max().item()) >= k:
                raise SystemExit(f"PARITY FAILURE ({name}): a literal index outside the list")
            rows = torch.repeat_interleave(torch.arange(n, device=dev), (first[0][1:] - first[0][:-1]))
            same_chunk = rows[1:] == rows[:-1]
            dp, dl = first[1][1:] - first[1][:-1], first[2][1:] - first[2][:-1]
            if not bool((~same_chunk | (dp > 0) | ((dp == 0) & (dl > 0))).all()):
                raise SystemExit(f"PARITY FAILURE ({name}): the entries of a chunk are not sorted by (pos, lit)")
            del rows, same_chunk, dp, dl
        shard.count_literals_async(stream, d_c.data_ptr(), k)
        torch.cuda.synchronize()
        if not torch.equal(torch.bincount(first[2].to(torch.int64), minlength=k), d_c):
            raise SystemExit(f"PARITY FAILURE ({name}): bincount(lit) against xsg_count_literals")
        d_pos.fill_(-1), d_lit.fill_(-1)
        find(total, a.grid)()
        torch.cuda.synchronize()
        if not (torch.equal(first[0], d_cp) and torch.equal(first[1], d_pos[:total]) and torch.equal(first[2], d_lit[:total])):
            raise SystemExit(f"PARITY FAILURE ({name}): grid {a.grid} differs from the default grid")
        if total:
            d_pos.fill_(-1), d_lit.fill_(-1)
            find(total - 1)()
            torch.cuda.synchronize()
            if not (int(d_st.item()) == xsg.STATUS_OVERFLOW and torch.equal(first[0], d_cp) and torch.equal(first[1][:-1], d_pos[:total - 1])
                    and torch.equal(first[2][:-1], d_lit[:total - 1]) and int(d_pos[total - 1].item()) == -1 and int(d_lit[total - 1].item()) == -1):
                raise SystemExit(f"PARITY FAILURE ({name}): the call clipped at total - 1")
        del first

        calls = {"count_literals (floor)": lambda: shard.count_literals_async(stream, d_c.data_ptr(), k), "two count passes (a)": two_counts,
                 "find": find(total), "find, sizing only": find(0)}
        host_calls = {"search offsets (b)": lambda: shard.search_u64_view(xsg.MATCH_BYTE_OFFSETS)}
        if total <= 1 << 28:  # (what the synchronous form keeps)
            host_calls["find, synchronous"] = shard.find_literals
        matches = int(shard.search_u64_view(xsg.MATCH_BYTE_OFFSETS).size)
        runs = {c: [] for c in list(calls) + list(host_calls)}
        for r in range(a.runs):
            for c, fn in (list(calls.items()) if r % 2 == 0 else list(calls.items())[::-1]):
                runs[c].append(device_ms(fn))
            for c, fn in host_calls.items():
                runs[c].append(host_ms(fn))
        floor = float(np.median(runs["count_literals (floor)"]))
        two = float(np.median(runs["two count passes (a)"]))
        for c, v in runs.items():
            emit({"shape": "128x16M", "list": name, "literals": k, "chunks": n, "bytes": int(ln.sum()), "total": total, "entry_bytes": 12 * total,
                  "leftmost_first_matches": matches, "call": c, "clock": "device (events)" if c in calls else "host (perf_counter, waits and fetches)",
                  "runs": a.runs, "calls_per_run": a.calls, **stats(v), "floor_ms": round(floor, 4), "two_counts_ms": round(two, 4),
                  "ratio_to_two_counts": round(float(np.median(v)) / two, 4)})
        del d_pos, d_lit
        torch.cuda.empty_cache()

    for name in a.lists.split(","):
        leg(name)


if __name__ == "__main__":
    main()
