#!/usr/bin/env python3
"""What xsg_count_literals_chunks costs (profiles/literal_matrix_ab.jsonl, DESIGN.md sections 3.5f and 5).

2 GiB of resident corpus.py text (the buffer of scripts/literal_counts_cost.py), bound three ways.  Every leg is --runs
interleaved runs; a run = --calls timed calls behind --warm untimed ones, its figure their median; a leg reports the
median of its runs and their min..max.
  floor   128 chunks of 16 MiB, the 8-word and the 300-word list.  Device time (events round the stream-ordered forms) of
          xsg_count_literals_async -- the floor: the parent's kernel, one flush per workgroup -- against
          xsg_count_literals_chunks_async with and without the touched list, and the memsets alone (hipMemsetAsync of
          n * k + k words).  `inside_floor_spread`: the matrix pass less the memset lies within the floor's own min..max.
  today   the same 128 chunks as a caller gets the matrix without this call: 128 x (rebind to one chunk +
          xsg_count_literals), host clock, against ONE synchronous xsg_count_literals_chunks (host clock, transfer of the
          matrix included).
  hard    the same bytes as 2^20 chunks of 2 KiB with the 8-word list (a 64 MB matrix) and as 2^16 chunks of 32 KiB with
          4096 seven-byte literals (a 2 GiB matrix, stream-ordered form only): every tile, or every other one, ends a chunk.  With the
          touched list and with XSG_LITMATRIX_TOUCHED=0 (every flush sweeps the histogram), and the memsets alone.
The device legs also time the pass without chunks_with and under --grids workgroups (XSG_LITMATRIX_GRID): what the
default grid and the summing of chunks_with in LDS were chosen by.  With --parent TREE (a checkout of the parent commit
with its library built) they time the parent build's same calls on the same binding, interleaved with this build's,
after comparing the two builds' count vectors, matrices and chunks_with word for word; a row of this build then carries
the parent's run medians of the same call (`same_run_ms`), the ratio to it (`ratio_to_same`) and the parent's own
max / min spread of it.  The runs alternate between the listed order and its reverse, so that neither build always
runs behind the other: with one build in both seats the second seat measured up to 0.5 % off the first."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

os.environ["XSG_TEST_HOOKS"] = "1"  # the A/B switches are re-read at every call
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "scripts")]


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's), for hipMemsetAsync"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            lib = C.CDLL(path)
            lib.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
            lib.hipMemsetAsync.restype = C.c_int
            return lib
    raise SystemExit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--templates", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--legs", default="floor,today,hard")
    ap.add_argument("--grids", type=int, nargs="*", default=[2048, 4096, 65536],
                    help="XSG_LITMATRIX_GRID values timed beside the default grid (64 workgroups per compute unit)")
    ap.add_argument("--parent", default="", help="a tree of the parent commit with x-search_amd/lib/libxsg.so built")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import corpus
    import literal_counts_cost
    import xsg
    dev = torch.device("cuda:0")
    hip = hip_runtime()
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
    shard = xsg.Shard(ctx, t.data_ptr(), cap, xsg.make_chunks(off, ln))
    pctx = pshard = None
    if a.parent:
        pxsg = literal_counts_cost.load_xsg(Path(a.parent).resolve(), "xsg_parent")
        pctx = pxsg.Context(0)
        pctx.set_pattern(b"x")
        pshard = pxsg.Shard(pctx, t.data_ptr(), cap, pxsg.make_chunks(off, ln))
    # a stream of the caller's for the stream-ordered forms, the events and everything that reads their results (the null
    # stream would stand for the context's own, which no event recorded here sees)
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
        """the median device time of --calls calls of fn (which enqueues on the current stream) behind --warm"""
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

    def host_ms(fn, warm, calls):
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))

    def interleaved(calls, measure):
        runs = {k: [] for k in calls}
        for r in range(a.runs):  # every other run in reverse order: no call always follows the same neighbour
            for k, fn in (list(calls.items()) if r % 2 == 0 else list(calls.items())[::-1]):
                runs[k].append(measure(fn))
        return runs

    def stats(v):
        return {"run_ms": [round(x, 4) for x in v], "ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def matrix_calls(shard, n, k, d_m, d_w, d_c):
        def matrix(touched, grid=None, with_chunks=True):
            def call():
                os.environ["XSG_LITMATRIX_TOUCHED"] = touched
                if grid:
                    os.environ["XSG_LITMATRIX_GRID"] = str(grid)
                try:
                    shard.count_literals_chunks_async(stream, d_m.data_ptr(), n * k, d_w.data_ptr() if with_chunks else 0, k if with_chunks else 0)
                finally:
                    os.environ.pop("XSG_LITMATRIX_GRID", None)
            return call

        def memsets():
            assert hip.hipMemsetAsync(d_m.data_ptr(), 0, 8 * n * k, stream) == 0
            assert hip.hipMemsetAsync(d_w.data_ptr(), 0, 8 * k, stream) == 0
        return {"count_literals (floor)": lambda: shard.count_literals_async(stream, d_c.data_ptr(), k),
                "matrix": matrix("1"), "matrix, no touched list": matrix("0"), "matrix, no chunks_with": matrix("1", None, False),
                **{f"matrix, grid {g}": matrix("1", g) for g in a.grids}, "memsets alone": memsets}

    def device_leg(what, name, lits, n, chunk_bytes):
        k = len(lits)
        ctx.set_literals(xsg.literal_list(lits), 0)
        d_m = torch.empty(n * k, dtype=torch.int64, device=dev)
        d_w = torch.empty(k, dtype=torch.int64, device=dev)
        d_c = torch.empty(k, dtype=torch.int64, device=dev)
        calls = matrix_calls(shard, n, k, d_m, d_w, d_c)
        if pshard:  # the parent's same calls, each beside this build's
            pctx.set_literals(xsg.literal_list(lits), 0)
            parent_calls = matrix_calls(pshard, n, k, d_m, d_w, d_c)
            paired = {}
            for call, fn in calls.items():
                if "grid" not in call and call != "memsets alone":
                    paired["parent " + call] = parent_calls[call]
                paired[call] = fn
            calls = paired
        # parity before any timing: both forms of the flush agree, and the columns sum to xsg_count_literals' counts
        calls["matrix"]()
        torch.cuda.synchronize()
        first, first_w = d_m.clone(), d_w.clone()
        calls["matrix, no touched list"]()
        calls["count_literals (floor)"]()
        torch.cuda.synchronize()
        if not (torch.equal(first, d_m) and torch.equal(first_w, d_w)):
            raise SystemExit(f"PARITY FAILURE ({what}, {name}): the two forms of the flush differ")
        if not torch.equal(first.view(n, k).sum(dim=0), d_c) or not torch.equal((first.view(n, k) > 0).sum(dim=0), first_w):
            raise SystemExit(f"PARITY FAILURE ({what}, {name}): column sums or chunks_with")
        if pshard:  # the two builds agree word for word: both forms of the flush, chunks_with, the count vector
            counts = d_c.clone()
            for form in ("parent matrix", "parent matrix, no touched list"):
                d_m.fill_(-1), d_w.fill_(-1), d_c.fill_(-1)
                calls[form]()
                calls["parent count_literals (floor)"]()
                torch.cuda.synchronize()
                if not (torch.equal(first, d_m) and torch.equal(first_w, d_w) and torch.equal(counts, d_c)):
                    raise SystemExit(f"PARITY FAILURE ({what}, {name}): {form} or its count vector differs from this build's")
            del counts
        runs = interleaved(calls, device_ms)
        floor = stats(runs["count_literals (floor)"])
        memset = float(np.median(runs["memsets alone"]))
        for call, v in runs.items():
            row = {"what": what, "list": name, "literals": k, "chunks": n, "chunk_bytes": chunk_bytes, "matrix_words": n * k,
                   "call": call, "clock": "device (events)", "runs": a.runs, "calls_per_run": a.calls, **stats(v)}
            if "parent " + call in runs:
                same = runs["parent " + call]
                row.update({"same_run_ms": [round(x, 4) for x in same], "same_ms": round(float(np.median(same)), 4), "ratio_to_same": round(row["ms"] / float(np.median(same)), 4),
                            "same_max_over_min": round(max(same) / min(same), 4)})
            if call.startswith("matrix"):
                m = row["ms"]
                row.update({"floor_ms": floor["ms"], "floor_min_ms": floor["min_ms"], "floor_max_ms": floor["max_ms"],
                            "memsets_ms": round(memset, 4), "memset_share": round(memset / m, 4),
                            "ratio_to_floor": round(m / floor["ms"], 4), "less_memsets_ms": round(m - memset, 4),
                            "inside_floor_spread": bool(floor["min_ms"] <= m - memset <= floor["max_ms"]),
                            "occurrences": int(d_c.sum().item()), "nonzero_words": int((first != 0).sum().item())})
            emit(row)
        del d_m, d_w, d_c, first
        torch.cuda.empty_cache()

    legs = a.legs.split(",")
    n = int(len(ln))
    if "floor" in legs:
        for name in ("8-words", "300-words"):
            device_leg("floor", name, named[name], n, 16 << 20)
    if "today" in legs:
        one = xsg.Shard(ctx, t.data_ptr(), cap, xsg.make_chunks(off[:1], ln[:1]))
        for name in ("8-words", "300-words"):
            lits = named[name]
            ctx.set_literals(xsg.literal_list(lits), 0)
            want = shard.count_literals_chunks()[0]

            def loop():
                rows = []
                for c in range(n):
                    one.rebind(t.data_ptr() + int(off[c]), (int(ln[c]) + 15) & ~15, xsg.make_chunks([0], [int(ln[c])]))
                    rows.append(one.count_literals())
                return rows
            if not np.array_equal(np.stack(loop()), want):
                raise SystemExit(f"PARITY FAILURE (today, {name}): the loop and the matrix differ")
            runs = interleaved({"128 x (rebind + count_literals)": loop, "matrix, synchronous": lambda: shard.count_literals_chunks()},
                               lambda fn: host_ms(fn, 1, max(a.calls // 2, 2)))
            base = float(np.median(runs["128 x (rebind + count_literals)"]))
            for call, v in runs.items():
                emit({"what": "today", "list": name, "literals": len(lits), "chunks": n, "call": call, "clock": "host", "runs": a.runs,
                      **stats(v), "loop_over_this": round(base / float(np.median(v)), 2)})
        one.close()
    if "hard" in legs:
        total = int(a.gib * 2**30)
        for name, lits, size in (("8-words", named["8-words"], 2048), ("4096-distinct-grams", named["4096-distinct-grams"], 32768)):
            m = total // size
            for sh in filter(None, (shard, pshard)):
                sh.rebind(t.data_ptr(), cap, xsg.make_chunks(np.arange(m, dtype=np.uint64) * size, np.full(m, size, dtype=np.uint64)))
            device_leg("hard", name, lits, m, size)


if __name__ == "__main__":
    main()
