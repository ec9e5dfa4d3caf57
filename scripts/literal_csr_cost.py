#!/usr/bin/env python3
"""What xsg_count_literals_csr costs (profiles/literal_csr_ab.jsonl, DESIGN.md sections 3.5g and 5).

2 GiB of resident corpus.py text (the buffer of scripts/literal_matrix_cost.py), bound three ways -- 128 chunks of 16 MiB,
2^16 chunks of 32 KiB, 2^20 chunks of 2 KiB -- under the 8-word, the 300-word and the 4096-literal list of
literal_counts_cost.lists() (--lists; `4096-text-cuts`, 4096 seven-byte cuts of the text, is the long list that occurs
everywhere: the list format's 32 KiB leave 4096 literals seven bytes each).  Every leg is
--runs interleaved runs (every other run in reverse order); a run = --calls timed calls behind --warm untimed ones, its
figure their median; a leg reports the median of its runs and their min..max.  Device time, events round the
stream-ordered forms on a stream of the caller's, memsets included:
  csr                     xsg_count_literals_csr_async with cap_entries = nnz (read once, untimed, from a sizing call)
  csr, no touched list    the same under XSG_LITMATRIX_TOUCHED=0: every count flush sweeps and every fill flush compacts the
                          whole histogram -- the A/B of the fill flush
  csr, grid G             the same under XSG_LITMATRIX_GRID=G (--grids): what the cap of the grid costs
  dense                   xsg_count_literals_chunks_async without chunks_with, where its n * k words fit --dense-gib
  count_literals (floor)  xsg_count_literals_async: one scan, one flush per workgroup; `two_scans_ms` is twice it
Before any timing the sparse result is checked for its form and, where the dense form ran, against it word for word; both
forms of the flush and two grids must agree bit for bit.  With --parent TREE (a checkout of the parent commit with its
library built) the parent's dense call runs interleaved with this build's on the same binding."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

os.environ["XSG_TEST_HOOKS"] = "1"  # the A/B switches are re-read at every call
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "scripts")]

SHAPES = {"128x16M": None, "64Kx32K": 32768, "1Mx2K": 2048}


def text_cuts(block, k, nbytes):
    """k distinct literals of nbytes cut from the text (no newline inside): unlike the 4096 random grams of
    literal_counts_cost.lists(), which the text never holds, these occur -- the rows of a long list get entries"""
    text = block.tobytes()
    rng = np.random.Generator(np.random.PCG64(4096))
    seen = {}
    while len(seen) < k:
        at = int(rng.integers(0, len(text) - nbytes))
        lit = text[at:at + nbytes]
        if b"\n" not in lit:
            seen.setdefault(lit, None)
    return list(seen)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--templates", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--shapes", default="128x16M,64Kx32K,1Mx2K")
    ap.add_argument("--lists", default="8-words,300-words,4096-distinct-grams")
    ap.add_argument("--grids", type=int, nargs="*", default=[2048], help="XSG_LITMATRIX_GRID values timed beside the default grid")
    ap.add_argument("--dense-gib", type=float, default=9.0, help="the dense form is timed where its matrix is at most this large")
    ap.add_argument("--cut-bytes", type=int, default=7, help="length of the literals of the list 4096-text-cuts")
    ap.add_argument("--parent", default="", help="a tree of the parent commit with x-search_amd/lib/libxsg.so built")
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
    named["4096-text-cuts"] = text_cuts(blocks[0], 4096, a.cut_bytes)
    ctx = xsg.Context(0)
    ctx.set_pattern(b"x")
    shard = xsg.Shard(ctx, t.data_ptr(), cap, xsg.make_chunks(off, ln))
    pctx = pshard = None
    if a.parent:
        pxsg = literal_counts_cost.load_xsg(Path(a.parent).resolve(), "xsg_parent")
        pctx = pxsg.Context(0)
        pctx.set_pattern(b"x")
        pshard = pxsg.Shard(pctx, t.data_ptr(), cap, pxsg.make_chunks(off, ln))
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

    def stats(v):
        return {"run_ms": [round(x, 4) for x in v], "ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def leg(shape, name, n, chunk_bytes):
        lits = named[name]
        k = len(lits)
        ctx.set_literals(xsg.literal_list(lits), 0)
        d_rp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(1, dtype=torch.int64, device=dev)
        d_c = torch.empty(k, dtype=torch.int64, device=dev)
        none = torch.empty(8, dtype=torch.int64, device=dev)
        shard.count_literals_csr_async(stream, d_rp.data_ptr(), n + 1, none.data_ptr(), none.data_ptr(), 0, d_st.data_ptr())  # the sizing pass
        torch.cuda.synchronize()
        nnz = int(d_rp[n].item())
        assert int(d_st.item()) == (xsg.STATUS_OVERFLOW if nnz else xsg.STATUS_OK)
        d_cols = torch.empty(nnz + 1, dtype=torch.int32, device=dev)
        d_vals = torch.empty(nnz + 1, dtype=torch.int64, device=dev)
        dense_ok = 8 * n * k <= a.dense_gib * 2**30
        d_m = torch.empty(n * k, dtype=torch.int64, device=dev) if dense_ok else None

        def csr(touched="1", grid=None):
            def call():
                os.environ["XSG_LITMATRIX_TOUCHED"] = touched
                if grid:
                    os.environ["XSG_LITMATRIX_GRID"] = str(grid)
                try:
                    shard.count_literals_csr_async(stream, d_rp.data_ptr(), n + 1, d_cols.data_ptr(), d_vals.data_ptr(), nnz, d_st.data_ptr())
                finally:
                    os.environ.pop("XSG_LITMATRIX_GRID", None)
                    os.environ["XSG_LITMATRIX_TOUCHED"] = "1"
            return call

        calls = {"count_literals (floor)": lambda: shard.count_literals_async(stream, d_c.data_ptr(), k), "csr": csr(),
                 "csr, no touched list": csr("0"), **{f"csr, grid {g}": csr("1", g) for g in a.grids}}
        if dense_ok:
            calls["dense"] = lambda: shard.count_literals_chunks_async(stream, d_m.data_ptr(), n * k, 0, 0)
            if pshard:
                pctx.set_literals(xsg.literal_list(lits), 0)
                calls["parent dense"] = lambda: pshard.count_literals_chunks_async(stream, d_m.data_ptr(), n * k, 0, 0)
        # parity before any timing
        calls["csr"]()
        torch.cuda.synchronize()
        assert int(d_st.item()) == xsg.STATUS_OK and int(d_rp[n].item()) == nnz and int(d_rp[0].item()) == 0
        first = (d_rp.clone(), d_cols[:nnz].clone(), d_vals[:nnz].clone())
        for other in [c for c in calls if c.startswith("csr, ")]:
            d_cols.fill_(-1), d_vals.fill_(-1)
            calls[other]()
            torch.cuda.synchronize()
            if not (torch.equal(first[0], d_rp) and torch.equal(first[1], d_cols[:nnz]) and torch.equal(first[2], d_vals[:nnz])):
                raise SystemExit(f"PARITY FAILURE ({shape}, {name}): '{other}' differs from 'csr'")
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (first[0][1:] - first[0][:-1]))
        flat = rows * k + first[1].to(torch.int64)
        if nnz and not (bool((flat[1:] > flat[:-1]).all()) and bool((first[2] > 0).all()) and int(first[1].max().item()) < k):
            raise SystemExit(f"PARITY FAILURE ({shape}, {name}): the result is no CSR matrix")
        calls["count_literals (floor)"]()
        torch.cuda.synchronize()
        sums = torch.zeros(k, dtype=torch.int64, device=dev).index_add_(0, first[1].to(torch.int64), first[2])
        if not torch.equal(sums, d_c):
            raise SystemExit(f"PARITY FAILURE ({shape}, {name}): column sums against xsg_count_literals")
        if dense_ok:
            for form in [c for c in calls if c.endswith("dense")]:
                d_m.fill_(-1)
                calls[form]()
                torch.cuda.synchronize()
                want = torch.zeros(n * k, dtype=torch.int64, device=dev)
                want[flat] = first[2]
                if not torch.equal(want, d_m):
                    raise SystemExit(f"PARITY FAILURE ({shape}, {name}): '{form}' differs from the sparse result")
                del want
        del rows, flat, sums
        runs = {c: [] for c in calls}
        for r in range(a.runs):
            for c, fn in (list(calls.items()) if r % 2 == 0 else list(calls.items())[::-1]):
                runs[c].append(device_ms(fn))
        floor = float(np.median(runs["count_literals (floor)"]))
        dense = float(np.median(runs["dense"])) if dense_ok else None
        for c, v in runs.items():
            row = {"shape": shape, "list": name, "literals": k, "chunks": n, "chunk_bytes": chunk_bytes, "matrix_words": n * k, "nnz": nnz,
                   "call": c, "clock": "device (events)", "runs": a.runs, "calls_per_run": a.calls, **stats(v), "floor_ms": round(floor, 4),
                   "two_scans_ms": round(2 * floor, 4), "ratio_to_two_scans": round(float(np.median(v)) / (2 * floor), 4)}
            if dense is not None:
                row.update({"dense_ms": round(dense, 4), "ratio_to_dense": round(float(np.median(v)) / dense, 4)})
            emit(row)
        del d_m, d_cols, d_vals, first
        torch.cuda.empty_cache()

    total = int(a.gib * 2**30)
    for shape in a.shapes.split(","):
        size = SHAPES[shape]
        if size is None:
            n, table = int(len(ln)), xsg.make_chunks(off, ln)
        else:
            n = total // size
            table = xsg.make_chunks(np.arange(n, dtype=np.uint64) * size, np.full(n, size, dtype=np.uint64))
        for sh in filter(None, (shard, pshard)):
            sh.rebind(t.data_ptr(), cap, table)
        for name in a.lists.split(","):
            leg(shape, name, n, size or (16 << 20))


if __name__ == "__main__":
    main()
